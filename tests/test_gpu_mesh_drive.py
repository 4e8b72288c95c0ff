"""GPU: nm_mesh_bind / nm_mesh_normals (csrc/nm_meshdrive.hip), the frame product and the layers above them against the numpy fp64
statement neuma_amd/extras/mesh_drive.py, on the meshes and clouds of tests/mesh_drive_cases.py.

Bounds (eps32 = 2^-23, u32 = eps32 / 2 the fp32 unit roundoff, eps64 = 2^-52; all figures but the measured one come from the yardstick):
  search     on the tie-free cases nm_knn's lists equal knn_brute's; d2 to 4 eps64 (three products, two sums).
  bind       the yardstick's bind is fed the GPU's own (idx, d2), so a last-bit tie in the search is not the bind's business.  col is
             equal.  Per vertex and entry, |c_j - c64_j| <= u32 |c64_j| (the one rounding to fp32) + 64 eps64 cond w^_j |y_j| |g|:
             c_j = w^_j (1 + y_j . g) and the fp64 solve of (M^ M^ + eps^2 I) loses at most its condition number (the yardstick's
             own, from the eigenvalues of M^) times eps64 of |g|, with 64 for the two 3x3 products, the k-term moment sums and the
             factorisation; w^_j has the rounding term alone plus 4 k eps64.  Where a vertex's largest entry bound exceeds
             1e-3 sum|c| nothing is claimed for it.  LEFT_OUT states the share that may be: none anywhere - the jittered-lattice
             cases with k = 8 and 16 included, whose condition numbers reach 1e2 (inside) and 1e6 (outside), and the rank-deficient
             cases, where cond = 1 / eps^2 = 1e10 but the damped direction carries y . g = 0 - except the four-neighbour case, where
             one vertex of 65 sits on a near-coplanar neighbourhood with |y . g| in the tens.
  positions  against the yardstick's drive with the yardstick's fp64 coefficients, per component:
             (k + 3) u32 sum_j |c_j| |u_j| (u_j = x_j - X_j: one rounding of the difference, one of the product, k of the
             running sum, one of c_j) + u32 |p| (the final add) + sum_j B_j |u_j| (B_j the bind bound above), times 1.01 for
             the second-order terms.  The identity motion gives V0 bit for bit.
  normals    the kernel and the yardstick are given the same fp32 positions (the GPU's own frame).  A corner's cross product
             carries at most 4 u32 (|a| |b|) per component (two differences, two products and their difference), the running sum of
             n of them (n - 1) u32 sum |cross| more; with sqrt(3) from components to length the sum s is off by at most
             d = sqrt(3) u32 (4 sum |a| |b| + (n - 1) sum |cross|), which turns it by at most d / |s| (doubled against the
             second-order term); the normalisation (a scaling, three squares, a root, a division) adds 8 eps32.  Where the bound
             exceeds 1 rad nothing is claimed: that happens to fans that cancel only.  The zero cases are exactly (0, 0, 0)."""
import numpy as np
import pytest
import torch

import mesh_drive_cases as mc
from gpu_util import dev, parity
from neuma_amd import _lib as L
from neuma_amd.extras import mesh_drive as md
from neuma_amd.mesh_drive import MeshDriver
from neuma_amd.particle_metrics import k_nearest_neighbors

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
PAIRS = [(n, k) for n in sorted(CASES) for k in CASES[n]["ks"]]
EPS = float(np.finfo(np.float32).eps)
U32 = EPS / 2
E64 = float(np.finfo(np.float64).eps)
LEFT_OUT = {("v65", 4): 1.0 / 65}          # the share of vertices for which the bind bound may claim nothing; 0 for every other case
MOTIONS = ("identity", "translation", "affine", "twist")


@pytest.fixture(scope="module")
def native():
    """(name, k) -> the driver bound on the GPU, with its arrays read back once"""
    out = {}
    for name, k in PAIRS:
        c = CASES[name]
        d = MeshDriver(c["V0"], c["tri"], c["X"], k=k, device=dev())
        out[name, k] = dict(driver=d, idx=d.idx.cpu().numpy(), d2=d.d2.cpu().numpy(), col=d.col.cpu().numpy(),
                            c=d.coeff.cpu().numpy(), w=d.weight.cpu().numpy())
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def yard(native):
    """(name, k) -> the yardstick's bind of the GPU's neighbour lists, and its entry bounds"""
    out = {}
    for (name, k), n in native.items():
        c = CASES[name]
        col, c64, w64, info = md.bind(c["V0"], c["X"], n["idx"], n["d2"])
        yn = np.sqrt((info["y"] ** 2).sum(2))
        gn = np.sqrt((info["g"] ** 2).sum(1))
        bc = U32 * np.abs(c64) + 64 * E64 * info["cond"][:, None] * w64 * yn * gn[:, None]
        out[name, k] = dict(col=col, c=c64, w=w64, info=info, bound_c=bc, bound_w=U32 * w64 + 4 * k * E64)
    return out


@pytest.mark.parametrize("name,k", [(n, k) for n, k in PAIRS if CASES[n]["tie_free"]])
def test_search_equals_the_brute_force_lists(native, name, k):
    c = CASES[name]
    idx, d2 = md.knn_brute(c["V0"], c["X"], k)
    assert np.array_equal(native[name, k]["idx"], idx)
    parity("mesh_drive", f"{name} k={k}: knn d2 (rel)", float((np.abs(native[name, k]["d2"] - d2) / np.maximum(d2, 1e-300)).max()), 4 * E64)


@pytest.mark.parametrize("name,k", PAIRS)
def test_bind_against_the_yardstick(native, yard, name, k):
    n, y = native[name, k], yard[name, k]
    assert n["col"].dtype == np.int32 and np.array_equal(n["col"], y["col"])
    claimed = y["bound_c"].max(1) <= 1e-3 * np.abs(y["c"]).sum(1)
    left = 1.0 - claimed.mean()
    print(f"{name} k={k}: cond max {y['info']['cond'].max():.3g}, sum|c| max {np.abs(y['c']).sum(1).max():.3g}, left out {left:.4f}")
    assert left <= LEFT_OUT.get((name, k), 0.0) + 1e-12
    assert np.isfinite(n["c"]).all() and np.isfinite(n["w"]).all()
    ratio = (np.abs(n["c"].astype(np.float64) - y["c"]) / y["bound_c"])[claimed]
    parity("mesh_drive", f"{name} k={k}: c / its bound (max over {int(claimed.sum())} vertices)", float(ratio.max()), 1.0)
    parity("mesh_drive", f"{name} k={k}: w^ / its bound", float((np.abs(n["w"].astype(np.float64) - y["w"]) / y["bound_w"]).max()), 1.0)


@pytest.mark.parametrize("name,k", PAIRS)
def test_positions_against_the_yardstick(native, yard, name, k):
    c, n, y = CASES[name], native[name, k], yard[name, k]
    d = n["driver"]
    for m in MOTIONS:
        x = mc.moved(c["X"], m)
        pos, nrm = d.frame(torch.from_numpy(x).to(dev()))
        pos = pos.cpu().numpy()
        assert pos.dtype == np.float32 and pos.shape == c["V0"].shape
        if m == "identity":
            assert pos.tobytes() == c["V0"].tobytes()
            continue
        want = md.drive(c["V0"], y["col"], y["c"], c["X"], x)
        u = np.abs(x.astype(np.float64) - c["X"].astype(np.float64))[y["col"]]                   # (V, k, 3)
        bound = 1.01 * ((k + 3) * U32 * (np.abs(y["c"])[:, :, None] * u).sum(1) + U32 * np.abs(want) + (y["bound_c"][:, :, None] * u).sum(1))
        claimed = y["bound_c"].max(1) <= 1e-3 * np.abs(y["c"]).sum(1)
        ratio = (np.abs(pos.astype(np.float64) - want) / np.maximum(bound, 1e-300))[claimed]
        parity("mesh_drive", f"{name} k={k} {m}: position / its bound (per component)", float(ratio.max()), 1.0)
        assert np.isfinite(pos).all()


def _normal_bound(P, tri):
    """(angle bound (V,), |s| (V,)) of the header, from the yardstick's own cross products of the fp32 positions P"""
    P = P.astype(np.float64)
    t = tri.astype(np.int64)
    s = np.zeros((len(P), 3))
    ab = np.zeros(len(P))
    cr = np.zeros(len(P))
    cnt = np.zeros(len(P))
    for c in range(3):
        iv, ia, ib = t[:, c], t[:, (c + 1) % 3], t[:, (c + 2) % 3]
        live = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
        a, b = P[ia] - P[iv], P[ib] - P[iv]
        x = np.cross(a, b) * live[:, None]
        np.add.at(s, iv, x)
        np.add.at(ab, iv, np.sqrt((a * a).sum(1) * (b * b).sum(1)) * live)
        np.add.at(cr, iv, np.sqrt((x * x).sum(1)))
        np.add.at(cnt, iv, 1.0)
    sl = np.sqrt((s * s).sum(1))
    dlt = np.sqrt(3.0) * U32 * (4 * ab + np.maximum(cnt - 1, 0) * cr)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sl > 0, 2 * dlt / sl, np.inf) + 8 * EPS, sl


@pytest.mark.parametrize("name", sorted(CASES))
def test_normals_against_the_yardstick(native, name):
    c = CASES[name]
    k = c["ks"][-1]
    d = native[name, k]["driver"]
    for m in ("identity", "affine", "twist"):
        pos, nrm = d.frame(torch.from_numpy(mc.moved(c["X"], m)).to(dev()))
        P, n = pos.cpu().numpy(), nrm.cpu().numpy().astype(np.float64)
        n64 = md.normals(P, c["tri"])
        bound, sl = _normal_bound(P, c["tri"])
        zero = sl == 0
        assert np.array_equal(n[zero], np.zeros((int(zero.sum()), 3))) and np.array_equal(n64[zero], np.zeros((int(zero.sum()), 3)))
        for v in c.get("zero_normals", ()):
            assert zero[v]
        ln = np.sqrt((n * n).sum(1))
        assert np.all(np.abs(ln[~zero] - 1.0) < 8 * EPS)
        ok = ~zero & (bound < 1.0)
        assert ok.sum() == (~zero).sum()                                       # no case here holds a fan that cancels only nearly
        if ok.any():
            ang = np.arctan2(np.sqrt((np.cross(n[ok], n64[ok]) ** 2).sum(1)), (n[ok] * n64[ok]).sum(1))
            parity("mesh_drive", f"{name} {m}: normal angle / its bound (max over {int(ok.sum())} vertices)", float((ang / bound[ok]).max()), 1.0)


def test_normals_of_a_fan_that_nearly_cancels_claim_nothing():
    """two opposite triangles that differ by one vertex moved by a few ulps: the sum is rounding, the bound says so, and the kernel
    still returns a unit vector or zero, never a NaN"""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32) * np.float32(0.3) + np.float32(0.5)
    P[3, 2] += np.float32(3e-7)
    tri = np.array([[0, 1, 2], [0, 4, 3]], dtype=np.int32)
    X = CASES["inside"]["X"]
    d = MeshDriver(P, tri, X, device=dev())
    pos, nrm = d.frame(torch.from_numpy(X).to(dev()))
    n = nrm.cpu().numpy()
    bound, sl = _normal_bound(pos.cpu().numpy(), tri)
    assert bound[0] > 1.0 and sl[0] > 0
    assert np.isfinite(n).all() and (abs(np.linalg.norm(n[0]) - 1) < 8 * EPS or not n[0].any())


@pytest.mark.parametrize("name,k", [("outside", 8), ("poles", 16), ("ties", 16), ("odd", 16), ("v257", 16)])
def test_two_calls_give_identical_bytes(native, name, k):
    c, n = CASES[name], native[name, k]
    again = MeshDriver(c["V0"], c["tri"], c["X"], k=k, device=dev())
    for a, b in ((again.col, n["col"]), (again.coeff, n["c"]), (again.weight, n["w"]), (again.idx, n["idx"])):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    x = torch.from_numpy(mc.moved(c["X"], "twist")).to(dev())
    p1, n1 = n["driver"].frame(x)
    p2, n2 = again.frame(x)
    assert p1.cpu().numpy().tobytes() == p2.cpu().numpy().tobytes() and n1.cpu().numpy().tobytes() == n2.cpu().numpy().tobytes()


def test_vertex_colours_follow_field_paint(native, yard):
    from neuma_amd.extras import field_paint as fp
    c, n, y = CASES["inside"], native["inside", 16], yard["inside", 16]
    x = mc.moved(c["X"], "twist")
    q = np.linalg.norm(x - c["X"], axis=1).astype(np.float32)
    bad = int(y["col"][5, 0])
    q[bad] = np.nan                                                            # no data: the vertices that read it turn grey
    pos, nrm, rgb = n["driver"].frame(torch.from_numpy(x).to(dev()), torch.from_numpy(q).to(dev()), (0.0, 0.5), "rainbow")
    g64 = md.vertex_values(n["w"].astype(np.float64), y["col"], q.astype(np.float64))
    want = fp.colors(torch.from_numpy(g64), (0.0, 0.5), "rainbow").numpy()
    reads = (y["col"] == bad).any(1)
    assert reads.any() and np.allclose(rgb.cpu().numpy()[reads], 0.5)
    # g carries (k + 2) u32 of its 16-term mean, the map's steepest knot-to-knot slope is 4 per unit t, t = g / 0.5
    parity("mesh_drive", "inside: vertex rgb (abs)", float(np.abs(rgb.cpu().numpy().astype(np.float64) - want)[~reads].max()),
           4 * (18 * U32 * np.nanmax(q) / 0.5) + 8 * EPS)
    _, _, auto = n["driver"].frame(torch.from_numpy(x).to(dev()), torch.from_numpy(np.nan_to_num(q)).to(dev()))
    assert tuple(auto.shape) == (642, 3) and float(auto.min()) >= 0 and float(auto.max()) <= 1 and float(auto.std()) > 0.05


def test_refused_inputs_launch_nothing():
    lib = L.lib()
    d = dev()
    V, N, k = 10, 100, 8
    verts, parts = torch.rand(V, 3, device=d), torch.rand(N, 3, device=d)
    idx, d2 = k_nearest_neighbors(verts[None], parts[None], k)
    col = torch.full((V, k), -7, dtype=torch.int32, device=d)
    co = torch.full((V, k), -7.0, device=d)
    we = torch.full((V, k), -7.0, device=d)
    s = L.stream_ptr(d)

    def bind(nv=V, n=N, kk=k, damping=1e-5, verts_p=verts.data_ptr()):
        return lib.nm_mesh_bind(nv, n, kk, damping, verts_p, parts.data_ptr(), idx.data_ptr(), d2.data_ptr(), col.data_ptr(), co.data_ptr(), we.data_ptr(), s)

    for kw in (dict(kk=0), dict(kk=17), dict(n=7), dict(damping=0.0), dict(damping=float("nan")), dict(damping=-1.0), dict(verts_p=None),
               dict(nv=2 ** 28, kk=8)):
        assert bind(**kw) == -1 and b"invalid argument" in lib.nm_last_error()
    nrm = torch.full((V, 3), -7.0, device=d)
    tri = torch.zeros(4, 3, dtype=torch.int32, device=d)
    vptr = torch.zeros(V + 1, dtype=torch.int32, device=d)
    vc = torch.zeros(12, dtype=torch.int32, device=d)
    assert lib.nm_mesh_normals(V, 4, verts.data_ptr(), None, vptr.data_ptr(), vc.data_ptr(), nrm.data_ptr(), s) == -1
    assert lib.nm_mesh_normals(V, -1, verts.data_ptr(), tri.data_ptr(), vptr.data_ptr(), vc.data_ptr(), nrm.data_ptr(), s) == -1
    assert lib.nm_mesh_normals(V, 4, verts.data_ptr(), tri.data_ptr(), vptr.data_ptr(), vc.data_ptr(), None, s) == -1
    torch.cuda.synchronize()
    for t in (col, co, we, nrm):
        assert bool((t == -7).all())                                           # nothing was written
    assert bind(nv=0) == 0 and lib.nm_mesh_normals(0, 0, None, None, None, None, None, s) == 0
    with pytest.raises(ValueError, match="bound to 100"):
        MeshDriver(verts.cpu().numpy(), np.zeros((0, 3), dtype=np.int32), parts.cpu().numpy(), k=k, device=d).frame(parts[:-1])


def test_an_adjacency_with_wild_entries_is_never_read_through():
    """the kernel checks every index it follows: corner ids and triangle indices far outside their arrays add zero"""
    d = dev()
    c = CASES["v65"]
    drv = MeshDriver(c["V0"], c["tri"], c["X"], device=d)
    tri = drv.triangles.clone()
    tri[3, 1] = 2 ** 30
    tri[5, 0] = -1
    vcorner = drv.vcorner.clone()
    vcorner[0] = 2 ** 30
    vcorner[1] = -5
    out = torch.empty(65, 3, device=d)
    L.check(L.lib().nm_mesh_normals(65, drv.T, L.ptr(drv.vertices), L.ptr(tri), L.ptr(drv.vptr), L.ptr(vcorner), L.ptr(out), L.stream_ptr(d)), "nm_mesh_normals")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    t = c["tri"].copy()
    keep = np.ones(len(t), dtype=bool)
    keep[[3, 5]] = False
    vc = drv.vcorner.cpu().numpy()
    far = ~np.isin(np.arange(65), c["tri"][[3, 5]].reshape(-1)) & ~np.isin(np.arange(65), c["tri"].reshape(-1)[vc[:2]])
    want = md.normals(c["V0"], t[keep])                                        # vertices away from the damage are as before
    got = out.cpu().numpy()
    ang = np.arccos(np.clip((got[far] * want[far]).sum(1), -1, 1))
    assert float(ang.max()) < 1e-3


def _png(path):
    from PIL import Image
    return np.array(Image.open(path)).astype(np.int32)


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """the tiny experiment of tests/test_gpu_entrypoints.py (1 frame) with stage A's init.pt, and a mesh in the frame of kernels.ply
    - an icosphere around the original particles' centre - as .ply and as .obj with a uv and a material; written once"""
    from test_gpu_entrypoints import _write_experiment
    from test_gpu_sh_deform import _write_init
    from neuma_amd import io as nio
    root = tmp_path_factory.mktemp("drive_exp")
    path, _ = _write_experiment(root, frames=1)
    _write_init(root, path)
    pts = nio.load_particles_ply(root / "raw" / "pcd.ply")
    sv, st = mc.icosphere(1)
    V0 = (pts.mean(0) + 0.5 * np.abs(pts - pts.mean(0)).max() * sv).astype(np.float32)
    nio.save_mesh_ply(root / "ball.ply", V0, None, None, st)
    obj = "mtllib ball.mtl\n" + "".join("v %.9g %.9g %.9g\n" % tuple(p) for p in V0) + "vt 0.5 0.5\nusemtl skin\n" + \
          "".join("f %d/1 %d/1 %d/1\n" % tuple(t + 1) for t in st)
    (root / "ball.obj").write_text(obj)
    return root, path, V0, st, obj


def test_render_drive_mesh_end_to_end(experiment):
    from neuma_amd import io as nio
    from neuma_amd.evaluate import main as render_main
    root, path, V0, st, obj = experiment
    res = root / "results"
    common = ["-c", str(path), "-es", "2", "-dv", "r_0", "--result_root", str(res)]
    render_main(common + ["-vn", "d", "--drive_mesh", str(root / "ball.ply"), "--color_by", "speed"])
    out = res / "tinyball-v1"
    assert sorted(p.name for p in (out / "driven_ball").iterdir()) == ["000.ply", "001.ply", "002.ply"]
    frames = [nio.read_ply_mesh(out / "driven_ball" / f"{i:03d}.ply") for i in range(3)]
    for i, (v, t) in enumerate(frames):
        assert np.array_equal(t, st) and len(v) == len(V0) and np.isfinite(v).all()
        assert "red" in nio.read_ply_vertices(out / "driven_ball" / f"{i:03d}.ply")
    assert frames[0][0].astype(np.float32).tobytes() == V0.tobytes()
    assert np.abs(frames[1][0] - frames[0][0]).max() > 0 and np.abs(frames[2][0] - frames[0][0]).max() > 0
    nrm = nio.read_ply_vertices(out / "driven_ball" / "002.ply")
    assert abs(float(np.sqrt(nrm["nx"] ** 2 + nrm["ny"] ** 2 + nrm["nz"] ** 2).min()) - 1.0) < 1e-5
    # without the flag: the same files as ever, images within the one 8-bit level two runs of one roll-out differ by
    render_main(common + ["-vn", "plain", "--color_by", "speed"])
    assert sorted(p.name for p in out.iterdir() if "plain" in p.name) == ["images_plain", "images_plain_speed"]
    assert sorted(p.name for p in out.iterdir() if p.name.startswith("driven")) == ["driven_ball"]
    names = sorted(p.name for p in (out / "images_d").glob("*.png"))
    assert names == sorted(p.name for p in (out / "images_plain").glob("*.png")) == [f"r_0_{i:03d}.png" for i in range(3)]
    for nm in names:
        assert np.abs(_png(out / "images_d" / nm) - _png(out / "images_plain" / nm)).max() <= 1
        assert np.abs(_png(out / "images_d_speed" / nm) - _png(out / "images_plain_speed" / nm)).max() <= 1
    # obj pass-through, a name of its own, no views at all
    render_main(["-c", str(path), "-es", "1", "--result_root", str(res), "-vn", "o", "--drive_mesh", str(root / "ball.obj"),
                 "--drive_mesh_name", "skin", "--drive_mesh_format", "obj", "--drive_mesh_k", "8"])
    assert sorted(p.name for p in (out / "driven_skin").iterdir()) == ["000.obj", "001.obj"]
    assert (out / "driven_skin" / "000.obj").read_text() == md.rewrite_obj(obj, V0)
    moved = (out / "driven_skin" / "001.obj").read_text()
    assert "usemtl skin" in moved and "vt 0.5 0.5" in moved and moved != (out / "driven_skin" / "000.obj").read_text()
    assert np.array_equal(md.read_obj(moved)[1], st)
    assert list((out / "images_o").glob("*.png")) == []


def test_inference_drive_mesh_on_one_of_two_objects(experiment):
    """the two-object scene of tests/test_gpu_entrypoints.py (one box above the other); the upper object carries `drive_mesh`"""
    import shutil
    import yaml
    from neuma_amd import io as nio, synth
    from neuma_amd.inference import main as inference_main
    root, path, V0, st, _ = experiment
    base = yaml.safe_load(path.read_text())
    raw, assets = root / "raw", root / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))}, raw / "plasticine_0300.pt")
    if not (assets / "tinycat").exists():
        shutil.copytree(assets / "tinyball", assets / "tinycat")
        for f in (assets / "tinycat").glob("particles.npz"):
            f.unlink()

    def obj(name, ckpt, lo):
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=dict(sh_degree=3),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 8.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"], views=["r_0"]))

    objects = [obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)]
    objects[0]["drive_mesh"] = str(root / "ball.ply")
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=32, eps=6e-7), objects=objects)
    demo = root / "multiobj-drive.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    res = root / "results-inf"
    inference_main(["-c", str(demo), "-s", "2", "-vn", "pair", "-dv", "r_0", "--save_gaussians", "pair", "--result_root", str(res)])
    out = res / "inference"
    assert sorted(p.name for p in out.iterdir() if p.name.startswith("driven")) == ["driven_tinyball"]
    assert sorted(p.name for p in (out / "driven_tinyball").iterdir()) == ["000.ply", "001.ply", "002.ply"]
    frames = [nio.read_ply_mesh(out / "driven_tinyball" / f"{i:03d}.ply") for i in range(3)]
    assert all(np.array_equal(t, st) and len(v) == len(V0) and np.isfinite(v).all() for v, t in frames)
    # the mesh went through the mapping of the object's Gaussian centres: into the upper box of the simulation
    lo, hi = np.array([0.25, 0.45, 0.25]), np.array([0.75, 0.95, 0.75])
    want0 = (V0.astype(np.float64) * 0.5 + lo)
    assert np.abs(frames[0][0] - want0).max() < 1e-6
    assert np.abs(frames[2][0] - frames[0][0]).max() > 0
    # and it stays with them: the mesh's centroid moves as the object's Gaussians' does, to a tenth of the step
    g0, g2 = (nio.load_gaussians_ply(out / "gaussians_pair" / f"{i:03d}.ply", 3).get_xyz.numpy() for i in (0, 2))
    mine = (g0 >= lo - 0.05).all(1) & (g0 <= hi + 0.05).all(1) & (g0[:, 1] > 0.5)
    dg, dm = (g2[mine] - g0[mine]).mean(0), (frames[2][0] - frames[0][0]).mean(0)
    assert np.abs(dg - dm).max() < 0.25 * np.abs(dg).max() + 1e-6
