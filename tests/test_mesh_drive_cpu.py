"""CPU: the fp64 statement of the driven meshes (neuma_amd/extras/mesh_drive.py) against what it claims, the OBJ pass-through, the
command line with --device cpu, and every refusal - the Python ones and, through ctypes, the two entry points' (they fail before
any device work, so no GPU is needed).  eps64 = 2^-52."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_drive_cases as mc
from neuma_amd.extras import mesh_drive as md

CASES = mc.all_cases()
E64 = float(np.finfo(np.float64).eps)
PAIRS = [(n, k) for n in sorted(CASES) for k in CASES[n]["ks"]]


@pytest.fixture(scope="module")
def bound():
    """(name, k) -> the yardstick's neighbour lists and bind, computed once"""
    out = {}
    for name, k in PAIRS:
        c = CASES[name]
        idx, d2 = md.knn_brute(c["V0"], c["X"], k)
        out[name, k] = (idx, d2) + md.bind(c["V0"], c["X"], idx, d2)
    return out


def _delta(info, eps=md.DEFAULT_DAMPING):
    """the damped share of r: sum_i eps^2 / (l_i^2 + eps^2) (r . e_i) e_i over the eigenpairs of M / tau (all of r where tau == 0)"""
    lam, vec = np.linalg.eigh(info["H"])
    share = eps * eps / (np.clip(lam, 0, None) ** 2 + eps * eps)
    share[info["tau"] <= 0] = 1.0
    ri = np.einsum("vai,va->vi", vec, info["r"])
    return np.einsum("vai,vi->va", vec, share * ri)


@pytest.mark.parametrize("name,k", PAIRS)
def test_neighbours_ascend_and_coefficients_sum_to_one(bound, name, k):
    idx, d2, col, c, w, info = bound[name, k]
    assert np.all(np.diff(d2, axis=1) >= 0) and np.array_equal(col, idx) and col.dtype == np.int32
    assert np.all(np.abs(w.sum(1) - 1.0) <= 4 * k * E64) and np.all(w >= 0)
    # sum c = 1 + (sum w^ y) . g, and the rounded first moment sum w^ y is at most k eps64 max|y| per term
    slack = 8 * k * E64 * (1.0 + (w * np.sqrt((info["y"] ** 2).sum(2))).sum(1) * np.sqrt((info["g"] ** 2).sum(1)) * k)
    assert np.all(np.abs(c.sum(1) - 1.0) <= slack)


@pytest.mark.parametrize("name,k", PAIRS)
def test_frame_zero_is_bitwise_the_input(bound, name, k):
    _, _, col, c, _, _ = bound[name, k]
    case = CASES[name]
    out = md.drive(case["V0"], col, c, case["X"], case["X"])
    assert out.astype(np.float32).tobytes() == case["V0"].tobytes()


@pytest.mark.parametrize("name,k", PAIRS)
def test_affine_reproduction_up_to_the_damped_share(bound, name, k):
    """sum c_j X_j = V0 - delta (with sum c_j = 1 that is the statement A V0 + b - (A - I) delta for every affine motion), delta from
    the yardstick's own eigenpairs.  Bound: the solve loses cond(M^ M^ + eps^2 I) eps64 of |r| (64 for the 3x3 products and the
    factorisation), the k-term sums 2 k eps64 of sum |c_j| |X_j|."""
    _, _, col, c, _, info = bound[name, k]
    case = CASES[name]
    X = case["X"].astype(np.float64)
    got = (c[:, :, None] * X[col]).sum(1)
    want = case["V0"].astype(np.float64) - _delta(info)
    rn = np.sqrt((info["r"] ** 2).sum(1))
    lim = 64 * E64 * info["cond"] * rn + 2 * k * E64 * (np.abs(c)[:, :, None] * np.abs(X[col])).sum(1).max(1) + 1e-300
    assert np.all(np.abs(got - want).max(1) <= lim), float((np.abs(got - want).max(1) / lim).max())
    # and through `drive`, on particles rounded to fp32 after the motion: each adds eps32 / 2 |x| through |c_j|
    for mname in ("translation", "affine"):
        A, b = mc.motions()[mname][1]
        x = mc.moved(case["X"], mname)
        pos = md.drive(case["V0"], col, c, case["X"], x)
        pred = want @ A.T + b - (want - case["V0"].astype(np.float64)) + 0.0          # A (V0 - delta) + b + delta
        lim2 = (lim * np.abs(A - np.eye(3)).sum() + np.abs(c).sum(1) * (2.0 ** -24) * np.abs(x).max() * 1.01 + 4 * k * E64 * np.abs(c).sum(1) * (np.abs(x).max() + 1))
        assert np.all(np.abs(pos - pred).max(1) <= lim2), (mname, float((np.abs(pos - pred).max(1) / lim2).max()))


def test_the_defaults_embed_a_lattice_cloud_well(bound):
    """the figures behind k = 16: inside a jittered lattice the fit is well conditioned and the coefficients stay small"""
    for k in (8, 16):
        _, _, _, c, _, info = bound["inside", k]
        assert info["cond"].max() < 1e4 and np.abs(c).sum(1).max() < 10.0
        assert np.abs(_delta(info)).max() < 1e-6 * np.abs(info["r"]).max()
    assert np.abs(bound["inside", 16][3]).sum(1).max() < 4.0


def test_sheet_moves_in_plane_and_keeps_its_offset(bound):
    """a coplanar cloud has no extent along its normal: the vertex follows the sheet's in-plane motion and carries its out-of-plane
    offset along unchanged - not rotated, not scaled, whatever the motion does along the normal"""
    case = CASES["sheet"]
    n = np.array([0.0, 0.0, 1.0])
    A = np.array([[0.6, -0.9, 0.7], [0.8, 0.5, -0.4], [0.0, 0.0, 3.0]])      # in-plane rotation, scale and shear; the third column is never seen
    b = np.array([0.1, -0.2, 0.3])
    X = case["X"].astype(np.float64)
    x = (X @ A.T + b).astype(np.float32)
    for k in case["ks"]:
        _, _, col, c, _, info = bound["sheet", k]
        assert np.all(info["eig"][:, 0] < 1e-12) and np.all(info["eig"][:, 1] > 1e-3)        # rank 2
        pos = md.drive(case["V0"], col, c, case["X"], x)
        V0 = case["V0"].astype(np.float64)
        off = (V0[:, 2] - 0.5)[:, None] * n
        want = (V0 - off) @ A.T + b + off
        lim = 1e-8 + np.abs(c).sum(1).max() * 2.0 ** -24 * np.abs(x).max()
        assert np.abs(pos - want).max() <= lim
    # tau == 0 (coincident particles): pure translation with the particles
    _, _, col, c, _, info = bound["coincident", 16]
    assert np.all(info["tau"] == 0) and np.all(info["g"] == 0) and np.allclose(c, 1.0 / 16, rtol=1e-15)
    cc = CASES["coincident"]
    pos = md.drive(cc["V0"], col, c, cc["X"], mc.moved(cc["X"], "affine"))
    shift = mc.moved(cc["X"], "affine")[0].astype(np.float64) - cc["X"][0].astype(np.float64)
    assert np.abs(pos - (cc["V0"].astype(np.float64) + shift)).max() <= 1e-14 * np.abs(shift).max() + 1e-15


def test_knn_brute_breaks_ties_by_index():
    case = CASES["ties"]
    idx, d2 = md.knn_brute(case["V0"], case["X"], 16)
    d = ((case["V0"].astype(np.float64)[:, None] - case["X"].astype(np.float64)[None]) ** 2).sum(2)
    for v in range(len(idx)):
        order = sorted(range(len(case["X"])), key=lambda i: (d[v, i], i))[:16]
        assert list(idx[v]) == order
    assert (np.diff(d2, axis=1) == 0).any()                                   # the case does hold exact ties


@pytest.mark.parametrize("name", sorted(CASES))
def test_corner_adjacency_ordering(name):
    case = CASES[name]
    tri, V = case["tri"], len(case["V0"])
    vptr, vcorner = md.corner_adjacency(tri, V)
    assert vptr.dtype == np.int32 and vcorner.dtype == np.int32 and len(vptr) == V + 1 and len(vcorner) == 3 * len(tri)
    assert vptr[0] == 0 and vptr[-1] == 3 * len(tri) and np.all(np.diff(vptr) >= 0)
    assert sorted(vcorner.tolist()) == list(range(3 * len(tri)))
    flat = tri.reshape(-1)
    for v in range(V):
        mine = vcorner[vptr[v]:vptr[v + 1]]
        assert np.all(flat[mine] == v) and np.all(np.diff(mine) > 0)


def test_normals_of_a_sphere_and_of_degenerate_fans():
    sv, st = mc.icosphere(3)
    n = md.normals(np.array([0.1, -0.2, 0.3]) + 0.7 * sv, st)
    assert np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() < 4 * E64
    assert np.arccos(np.clip((n * sv).sum(1), -1, 1)).max() < 0.02            # outward, radial to the facet size
    pv, pt = mc.uv_sphere(100, 5)
    npole = md.normals(pv, pt)
    assert np.abs(npole[0] - [0, 0, 1]).max() < 1e-12 and np.abs(npole[-1] - [0, 0, -1]).max() < 1e-12
    odd = CASES["odd"]
    no = md.normals(odd["V0"], odd["tri"])
    for v in odd["zero_normals"]:
        assert np.array_equal(no[v], np.zeros(3))
    assert abs(np.linalg.norm(no[3]) - 1.0) < 4 * E64                          # the repeated-index triangle adds nothing to vertex 3
    P = odd["V0"].astype(np.float64)
    only = np.cross(P[0] - P[3], P[2] - P[3])
    assert np.abs(no[3] - only / np.linalg.norm(only)).max() < 1e-14
    assert np.array_equal(md.normals(CASES["no_triangles"]["V0"], CASES["no_triangles"]["tri"]), np.zeros((12, 3)))
    bad = P.copy()
    bad[0, 0] = np.inf
    assert np.array_equal(md.normals(bad, odd["tri"])[0], np.zeros(3))


def test_obj_pass_through_keeps_everything_but_positions_and_normals():
    v, t = md.read_obj(mc.OBJ_TEXT)
    assert v.shape == (5, 3) and t.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 4]]
    new = (v + [0.125, 0.0, -0.25]).astype(np.float32)
    out = md.rewrite_obj(mc.OBJ_TEXT, new)
    src, dst = mc.OBJ_TEXT.splitlines(keepends=True), out.splitlines(keepends=True)
    assert not any(line.split()[:1] == ["vn"] for line in dst)
    src = [line for line in src if line.split()[:1] != ["vn"]]
    assert len(src) == len(dst)
    seen = 0
    for a, b in zip(src, dst):
        head = a.split()[:1]
        if head == ["v"]:
            tok = b.split()
            assert tok[0] == "v" and np.array_equal(np.array(tok[1:4], dtype=np.float64).astype(np.float32), new[seen])
            assert tok[4:] == a.split()[4:]                                    # a vertex colour stays
            seen += 1
        elif head == ["f"]:
            assert b == {"f 1/1/1 2/2/1  3/3/2 4/4/2\n": "f 1/1 2/2  3/3 4/4\n", "f -1//2 1//1 2//1\n": "f -1 1 2\n", "f -5/1 -4/2 -1/3\n": "f -5/1 -4/2 -1/3\n"}[a]
        else:
            assert a == b                                                      # comments, mtllib, o, vt, g, usemtl, s, the blank line
    assert seen == 5
    v2, t2 = md.read_obj(out)
    assert np.array_equal(v2.astype(np.float32), new) and np.array_equal(t2, t)
    assert md.rewrite_obj(mc.OBJ_TEXT.replace("\n", "\r\n"), new).count("\r\n") == out.count("\n")
    with pytest.raises(ValueError):
        md.rewrite_obj(mc.OBJ_TEXT, new[:4])


def test_mesh_driver_on_the_cpu_runs_the_yardstick(bound):
    from neuma_amd.mesh_drive import MeshDriver
    case = CASES["v65"]
    d = MeshDriver(case["V0"], case["tri"], case["X"], k=8, device="cpu")
    assert "V = 65" in d.describe() and "k = 8" in d.describe() and "max sum|c|" in d.describe()
    pos, nrm = d.frame(torch.from_numpy(case["X"]))
    assert pos.dtype == torch.float32 and pos.numpy().tobytes() == case["V0"].tobytes()
    x = mc.moved(case["X"], "twist")
    pos, nrm, rgb = d.frame(x, values=np.linalg.norm(x - case["X"], axis=1), colormap="heat")
    _, _, col, c, w, _ = bound["v65", 8]
    assert np.array_equal(pos.numpy(), md.drive(case["V0"], col, c, case["X"], x).astype(np.float32))
    assert tuple(rgb.shape) == (65, 3) and float(rgb.min()) >= 0 and float(rgb.max()) <= 1 and float(rgb.std()) > 0
    assert np.abs(np.linalg.norm(nrm.numpy(), axis=1)[np.diff(md.corner_adjacency(case["tri"], 65)[0]) > 0] - 1).max() < 1e-6


def test_command_line_on_the_cpu(tmp_path, capsys):
    from neuma_amd import io as nio
    from neuma_amd.mesh_drive import main
    case = CASES["inside"]
    X = case["X"]
    (tmp_path / "m.obj").write_text(mc.OBJ_TEXT)
    nio.save_particles_ply(tmp_path / "rest.ply", X)
    states = tmp_path / "states"
    states.mkdir()
    for i, m in enumerate(("identity", "translation", "twist")):
        nio.save_particles_ply(states / f"{i:03d}.ply", mc.moved(X, m))
    nio.save_particles_ply(states / "notes.ply", X)                             # not a frame
    base = ["--mesh", str(tmp_path / "m.obj"), "--rest", str(tmp_path / "rest.ply"), "--states", str(states), "--device", "cpu"]
    assert main(base + ["-o", str(tmp_path / "out_obj"), "--format", "obj", "--k", "8"]) == 0
    said = capsys.readouterr().out.splitlines()
    assert said[0].startswith("mesh drive: V = 5, T = 4, k = 8") and len(said) == 4
    assert "largest edge / rest = 1 " in said[1] and "V = 5, T = 4" in said[3]
    assert sorted(p.name for p in (tmp_path / "out_obj").iterdir()) == ["000.obj", "001.obj", "002.obj"]
    v0, t0 = md.read_obj(mc.OBJ_TEXT)
    first = (tmp_path / "out_obj" / "000.obj").read_text()
    assert first == md.rewrite_obj(mc.OBJ_TEXT, v0.astype(np.float32))          # frame 0: the source, positions bitwise
    v1, t1 = md.read_obj((tmp_path / "out_obj" / "001.obj").read_text())
    assert np.array_equal(t1, t0) and np.abs(v1 - (v0.astype(np.float32).astype(np.float64) + mc.SHIFT)).max() < 2e-6
    assert "usemtl blue" in first and "vt 1 1" in first and "vn" not in first
    assert main(base + ["-o", str(tmp_path / "out_ply")]) == 0
    for i in range(3):
        v, t = nio.read_ply_mesh(tmp_path / "out_ply" / f"{i:03d}.ply")
        assert np.array_equal(t, t0) and len(v) == 5 and "nx" in nio.read_ply_vertices(tmp_path / "out_ply" / f"{i:03d}.ply")
    assert np.array_equal(nio.read_ply_mesh(tmp_path / "out_ply" / "000.ply")[0].astype(np.float32), v0.astype(np.float32))
    # a .ply mesh in, obj out: the plain writer
    nio.save_mesh_ply(tmp_path / "m.ply", v0, None, None, t0)
    assert main(["--mesh", str(tmp_path / "m.ply")] + base[2:] + ["-o", str(tmp_path / "out2"), "--format", "obj"]) == 0
    assert "vn " in (tmp_path / "out2" / "002.obj").read_text()
    with pytest.raises(FileNotFoundError):
        main(base[:4] + ["--states", str(tmp_path), "--device", "cpu", "-o", str(tmp_path / "none")])


def test_python_refusals():
    from neuma_amd.mesh_drive import MeshDriver
    case = CASES["v65"]
    V0, tri, X = case["V0"], case["tri"], case["X"]
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="k ="):
            MeshDriver(V0, tri, X, k=k, device="cpu")
    with pytest.raises(ValueError, match="fewer than k"):
        MeshDriver(V0, tri, X[:7], k=8, device="cpu")
    for damping in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="damping"):
            MeshDriver(V0, tri, X, damping=damping, device="cpu")
    bad = V0.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="vertices"):
        MeshDriver(bad, tri, X, device="cpu")
    badx = X.copy()
    badx[0, 0] = np.inf
    with pytest.raises(ValueError, match="rest particles"):
        MeshDriver(V0, tri, badx, device="cpu")
    for t in (np.array([[0, 1, 65]]), np.array([[-1, 1, 2]]), np.array([[0.0, 1.0, 2.0]]), np.array([[0, 1, 2, 3]])):
        with pytest.raises(ValueError, match="triangles"):
            MeshDriver(V0, t, X, device="cpu")
    with pytest.raises(ValueError):
        MeshDriver(V0[:, :2], tri, X, device="cpu")
    d = MeshDriver(V0, tri, X, device="cpu")
    with pytest.raises(ValueError, match="bound to 1728"):
        d.frame(X[:-1])
    with pytest.raises(ValueError, match="non-finite"):
        d.frame(badx)
    with pytest.raises(ValueError, match="values"):
        d.frame(X, values=np.zeros(5))


def _last(lib):
    return lib.nm_last_error().decode()


def test_entry_points_refuse_before_any_device_work():
    """every refusal of nm_mesh_bind / nm_mesh_normals returns NM_ERR_INVALID with a message; the pointers are never followed
    (they point nowhere), so this runs without a GPU"""
    from neuma_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)

    def bind(nv=10, n=100, k=8, damping=1e-5, ptrs=(p,) * 7):
        return lib.nm_mesh_bind(nv, n, k, damping, *ptrs, None)

    for kw, word in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(k=-3), "k = -3"), (dict(n=7), "n_particles = 7"), (dict(nv=-1), "n_verts = -1"),
                     (dict(nv=2 ** 27, n=2 ** 20, k=16), "int32"), (dict(damping=0.0), "damping"), (dict(damping=-1.0), "damping"),
                     (dict(damping=float("nan")), "damping"), (dict(damping=float("inf")), "damping")):
        assert bind(**kw) == -1 and word in _last(lib), (kw, _last(lib))
    for i in range(7):
        assert bind(ptrs=tuple(None if j == i else p for j in range(7))) == -1 and "null pointer" in _last(lib)
    assert bind(nv=0, ptrs=(None,) * 7) == 0                                    # n_verts == 0: a no-op

    def normals(nv=10, nt=5, ptrs=(p,) * 5):
        return lib.nm_mesh_normals(nv, nt, *ptrs, None)

    assert normals(nv=-1) == -1 and "n_verts = -1" in _last(lib)
    assert normals(nt=-2) == -1 and "n_tris = -2" in _last(lib)
    assert normals(nt=2 ** 30) == -1 and "int32" in _last(lib)
    for i in range(5):
        assert normals(ptrs=tuple(None if j == i else p for j in range(5))) == -1 and "NULL" in _last(lib).upper()
    assert normals(nv=0, ptrs=(None,) * 5) == 0
