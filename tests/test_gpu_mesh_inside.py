"""GPU: the point-in-mesh kernel of csrc/nm_mesh.hip (nm_points_in_mesh) through neuma_amd.mesh_inside - mask for mask
against the CPU ray-parity test of extras.mesh_sampling on closed, nested, open and degenerate meshes, on points that sit
exactly on vertices, edges and faces (and a few ulp away), at 10^6 triangles against the analytic sphere, for
reproducibility, edge cases and ABI checks, and through prepare_simulation_data against the CPU sampler."""

import numpy as np
import pytest
import torch

from gpu_util import dev, measured

pytestmark = pytest.mark.gpu


def _mi():
    from neuma_amd import mesh_inside
    return mesh_inside


def _cpu():
    from neuma_amd.extras import mesh_sampling
    return mesh_sampling


# ------------------------------------------------------------------ meshes

def uv_sphere(n_lat, n_lon, r=1.0, center=(0.0, 0.0, 0.0)):
    """closed UV sphere: 2 poles + (n_lat - 1) rings of n_lon vertices, 2 n_lon (n_lat - 1) triangles, outward winding"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.repeat(np.cos(th)[:, None], n_lon, 1)], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * r + np.asarray(center)
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    top = np.stack([np.zeros(n_lon, int), idx[0], nxt[0]], -1)
    bot = np.stack([np.full(n_lon, len(v) - 1), nxt[-1], idx[-1]], -1)
    a, b, c, d = idx[:-1], idx[1:], nxt[1:], nxt[:-1]
    mid = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, np.concatenate([top, mid, bot]).astype(np.int64)


def torus(n_u, n_v, R=1.0, r=0.35):
    u = 2 * np.pi * np.arange(n_u) / n_u
    w = 2 * np.pi * np.arange(n_v) / n_v
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    i = np.arange(n_u)[:, None] * n_v + np.arange(n_v)[None]
    j = np.roll(i, -1, 0)
    k = np.roll(i, -1, 1)
    l = np.roll(j, -1, 1)
    t = np.concatenate([np.stack([i, j, l], -1).reshape(-1, 3), np.stack([i, l, k], -1).reshape(-1, 3)])
    return v, t


def open_cylinder(n, m, r=0.5, h=1.5):
    """open tube (no caps) along x, so that the +z rays cross its wall"""
    ph = 2 * np.pi * np.arange(n) / n
    z = np.linspace(-h / 2, h / 2, m)
    v = np.stack([np.repeat(r * np.cos(ph)[None], m, 0), np.repeat(r * np.sin(ph)[None], m, 0), np.repeat(z[:, None], n, 1)], -1)
    i = np.arange(m - 1)[:, None] * n + np.arange(n)[None]
    k = (np.arange(m - 1)[:, None] * n + (np.arange(n)[None] + 1) % n)
    t = np.concatenate([np.stack([i, i + n, k + n], -1).reshape(-1, 3), np.stack([i, k + n, k], -1).reshape(-1, 3)])
    return v.reshape(-1, 3)[:, [2, 1, 0]].copy(), t


BOX_V = np.array([[0, 0, 0], [2, 0, 0], [2, 1, 0], [0, 1, 0], [0, 0, 1], [2, 0, 1], [2, 1, 1], [0, 1, 1]], float)
BOX_T = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5],
                  [3, 0, 4], [3, 4, 7]])


def _check_equal(pts, v, t, label):
    got = _mi().points_in_mesh(pts, v, t, dev())
    ref = _cpu().points_in_mesh(pts, v, t)
    assert got.dtype == bool and got.shape == ref.shape
    assert measured(int((got != ref).sum()), f"{label}: masks differing from the CPU test") <= 0
    return got


def _check_sampling(v, t, label, res_vol=24, res_uni=16):
    for mode, res in (("volumetric", res_vol), ("uniform", res_uni)):
        got = _mi().sample_mesh_points(v, t, mode, res, seed=3, device=dev())
        ref = _cpu().sample_mesh_points(v, t, mode, res, seed=3)
        assert got.shape == ref.shape and np.array_equal(got, ref), f"{label} {mode}"      # same points, same order


# ------------------------------------------------------------------ 1. exactness against the CPU test

def test_closed_box_of_the_io_test():
    p = np.array([[1.0, 0.5, 0.5], [2.5, 0.5, 0.5], [0.2, 0.9, 0.1], [1.0, 0.5, -0.1], [1.0, 0.5, 1.1]])
    assert _check_equal(p, BOX_V, BOX_T, "box").tolist() == [True, False, True, False, False]
    _check_sampling(BOX_V, BOX_T, "box", 10, 8)
    assert len(_mi().sample_mesh_points(BOX_V, BOX_T, "volumetric", 10, device=dev())) == 10 * 5 * 5


@pytest.mark.parametrize("name", ["sphere", "torus", "sphere_far"])
def test_closed_meshes(name):
    if name == "torus":
        v, t = torus(48, 24)
    else:
        v, t = uv_sphere(30, 48)                                     # 2 784 triangles
        if name == "sphere_far":
            v = v + 1e3
    assert len(t) > 2000
    _check_sampling(v, t, name)


def test_nested_shells_leave_the_hollow_outside():
    vo, to = uv_sphere(24, 40)
    vi, ti = uv_sphere(16, 28, r=0.5)
    v, t = np.concatenate([vo, vi]), np.concatenate([to, ti + len(vo)])
    pts = _cpu().mesh_candidate_points(v, "volumetric", 24)
    got = _check_equal(pts, v, t, "nested")
    r = np.linalg.norm(pts, axis=1)
    assert not got[r < 0.45].any() and got[(r > 0.55) & (r < 0.95)].all() and not got[r > 1.0].any()
    _check_sampling(v, t, "nested")


def test_open_cylinder():
    v, t = open_cylinder(40, 12)
    _check_sampling(v, t, "open cylinder")


def test_vertical_triangles_and_repeated_vertices():
    vs, ts = uv_sphere(16, 24)
    # vertical fins (zero area in xy, axis-aligned and diagonal), a triangle with a repeated index, duplicated vertices
    fins = np.array([[0.1, -0.8, -0.5], [0.1, 0.8, -0.5], [0.1, 0.0, 0.7], [-0.6, -0.6, -0.3], [0.6, 0.6, -0.3], [0.0, 0.0, 0.6],
                     [0.3, 0.2, 0.1], [0.1, 0.2, 0.4]], float)
    v = np.concatenate([vs, fins, vs[:30]])                                  # vs[:30] repeated as new vertices
    n0 = len(vs)
    extra = [[n0, n0 + 1, n0 + 2], [n0 + 3, n0 + 4, n0 + 5], [n0 + 6, n0 + 6, n0 + 7], [n0 + 6, n0 + 7, n0 + 6]]
    dup = ts[:40].copy()
    dup[dup < 30] += n0 + len(fins)                                         # the same triangles again through the copies
    t = np.concatenate([ts, np.asarray(extra), dup])
    _check_sampling(v, t, "degenerate", 20, 14)


def test_query_points_on_vertices_and_edges_and_a_few_ulp_away():
    """The mesh is built around the OFFSET query points: vertices exactly on their xy, edges through them, and copies moved by
    1 and 3 ulp; a far vertex fixes the span of the offset (so the points fed to both paths are known exactly)."""
    cpu = _cpu()
    far = np.array([[100.0, -100.0, 0.0]])
    base = np.array([[0.25, 0.5, 0.0], [0.625, 0.375, 0.0], [0.1, 0.7, 0.0]])
    q = cpu.ray_offset_points(base, far)                                   # span = 100 here and below (the far vertex is the max)
    verts, tris = [far[0]], []

    def pyramid(cx, cy, h=0.05):
        """closed pyramid with its apex at (cx, cy, 0.8) and base corners at (cx +- h, cy +- h, 0.2); an edge-aligned twin"""
        i = len(verts)
        verts.extend([[cx, cy, 0.8], [cx - h, cy - h, 0.2], [cx + h, cy - h, 0.2], [cx + h, cy + h, 0.2], [cx - h, cy + h, 0.2]])
        tris.extend([[i, i + 1, i + 2], [i, i + 2, i + 3], [i, i + 3, i + 4], [i, i + 4, i + 1], [i + 1, i + 3, i + 2], [i + 1, i + 4, i + 3]])

    def diamond(cx, cy, h=0.04):
        """closed octahedron whose xy edges run through (cx, cy): vertices at (cx, cy +- h) and (cx +- h, cy)"""
        i = len(verts)
        verts.extend([[cx, cy - h, 0.5], [cx + h, cy, 0.5], [cx, cy + h, 0.5], [cx - h, cy, 0.5], [cx, cy, 0.9], [cx, cy, 0.1]])
        for a, b in ((0, 1), (1, 2), (2, 3), (3, 0)):
            tris.extend([[i + a, i + b, i + 4], [i + b, i + a, i + 5]])

    pts = []
    for k, (x, y, _) in enumerate(q):
        for du in (0, 1, 3):
            px, py = x, y
            for _ in range(du):
                px, py = np.nextafter(px, np.inf), np.nextafter(py, -np.inf)
            (pyramid if k % 2 == 0 else diamond)(px, py)
        for z in (0.3, 0.5, 0.85):
            pts.append([base[k, 0], base[k, 1], z])
    verts, tris = np.asarray(verts, float), np.asarray(tris)
    assert float(np.abs(verts).max()) == 100.0
    _check_equal(np.asarray(pts), verts, tris, "on vertices / edges")


def test_points_whose_z_equals_a_face_exactly():
    """pz set to the fp64 z the formula computes for that face at the offset point, and to its neighbours"""
    cpu = _cpu()
    v, t = uv_sphere(10, 14)
    rng = np.random.default_rng(7)
    xy = rng.uniform(-0.6, 0.6, (40, 2))
    base = np.concatenate([xy, np.zeros((40, 1))], 1)
    q = cpu.ray_offset_points(base, v)
    a, b, c = (v[t[:, k]] for k in range(3))
    d = (b[:, 1] - c[:, 1]) * (a[:, 0] - c[:, 0]) + (c[:, 0] - b[:, 0]) * (a[:, 1] - c[:, 1])
    pts = []
    for i in range(len(q)):
        px, py = q[i, 0], q[i, 1]
        l0 = ((b[:, 1] - c[:, 1]) * (px - c[:, 0]) + (c[:, 0] - b[:, 0]) * (py - c[:, 1])) / d
        l1 = ((c[:, 1] - a[:, 1]) * (px - c[:, 0]) + (a[:, 0] - c[:, 0]) * (py - c[:, 1])) / d
        l2 = 1.0 - l0 - l1
        z = l0 * a[:, 2] + l1 * b[:, 2] + l2 * c[:, 2]
        for j in np.nonzero((np.abs(d) > 1e-300) & (l0 >= 0) & (l1 >= 0) & (l2 >= 0))[0]:
            for zz in (z[j], np.nextafter(z[j], np.inf), np.nextafter(z[j], -np.inf)):
                pts.append([base[i, 0], base[i, 1], zz])
    pts = np.asarray(pts)
    assert len(pts) >= 6 * 40
    _check_equal(pts, v, t, "pz on a face")


# ------------------------------------------------------------------ 2. scale: 10^6 triangles against the analytic sphere

@pytest.mark.parametrize("res", [36, 60])
def test_million_triangle_sphere_against_the_analytic_sphere(res):
    n_lat, n_lon = 500, 1000
    v, t = uv_sphere(n_lat, n_lon)
    assert len(t) == 998_000
    cpu = _cpu()
    pts = cpu.mesh_candidate_points(v, "volumetric", res)
    got = _mi().points_in_mesh(pts, v, t, dev())
    r = np.linalg.norm(cpu.ray_offset_points(pts, v), axis=1)
    # every vertex lies on the unit sphere; a planar facet dips below it by at most its circumradius' sagitta, and each
    # facet fits in a circle of angular radius <= one longitude step
    band = 1.0 - np.cos(2 * np.pi / n_lon)
    sure = np.abs(r - 1.0) > band
    assert sure.sum() > 0.99 * len(pts)
    assert measured(int((got[sure] != (r[sure] < 1.0)).sum()), f"res {res}: points off the analytic sphere") <= 0
    samp = _mi().sample_mesh_points(v, t, "volumetric", res, device=dev())
    assert np.array_equal(samp, pts[got])


# ------------------------------------------------------------------ 3. determinism, edge cases, errors, the ABI

def test_two_calls_give_identical_bytes():
    mi, cpu = _mi(), _cpu()
    v, t = torus(64, 32)
    pts = cpu.ray_offset_points(cpu.mesh_candidate_points(v, "uniform", 40, seed=1), v)
    P = torch.from_numpy(pts).to(dev())
    V = torch.from_numpy(v).to(dev())
    T = torch.from_numpy(t.astype(np.int32)).to(dev())
    a = mi.inside_native(P, V, T).cpu().numpy()
    b = mi.inside_native(P, V, T).cpu().numpy()
    assert a.tobytes() == b.tobytes() and set(np.unique(a)) <= {0, 1} and 0 < a.sum() < len(a)


def test_edge_cases_and_errors():
    mi = _mi()
    p = np.random.default_rng(0).uniform(-1, 1, (100, 3))
    v, t = uv_sphere(8, 12)
    assert not mi.points_in_mesh(p, v, np.zeros((0, 3), np.int64), dev()).any()
    assert mi.points_in_mesh(np.zeros((0, 3)), v, t, dev()).shape == (0,)
    for bad in (np.array([[0, 1, len(v)]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError):
            mi.points_in_mesh(p, v, bad, dev())
    with pytest.raises(ValueError):
        mi.points_in_mesh(p[:, :2], v, t, dev())
    with pytest.raises(ValueError):
        mi.points_in_mesh(p, v[:, :2], t, dev())
    with pytest.raises(ValueError):
        mi.points_in_mesh(p, v, t[:, :2], dev())
    with pytest.raises(ValueError):
        mi.points_in_mesh(p, v, t.astype(float), dev())
    from neuma_amd import NeumaHipError
    with pytest.raises(NeumaHipError):
        mi.points_in_mesh(p, v, t, "cpu")


def test_abi_rejects_bad_sizes_and_small_workspaces():
    from neuma_amd import _lib as L
    lib = L.lib()
    assert lib.nm_mesh_inside_workspace(-1, 10) == 0 and lib.nm_mesh_inside_workspace(10, -1) == 0
    assert lib.nm_mesh_inside_workspace((1 << 27) + 1, 10) == 0
    need = int(lib.nm_mesh_inside_workspace(12, 5))
    assert need > 0
    V = torch.from_numpy(BOX_V).to(dev())
    T = torch.from_numpy(BOX_T.astype(np.int32)).to(dev())
    P = torch.zeros(5, 3, dtype=torch.float64, device=dev())
    out = torch.full((5,), 7, dtype=torch.uint8, device=dev())
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    s = L.stream_ptr(dev())
    args = (V.data_ptr(), T.data_ptr(), P.data_ptr(), out.data_ptr())
    assert lib.nm_points_in_mesh(8, -1, 5, *args, ws.data_ptr(), need, s) == -1
    assert lib.nm_points_in_mesh(-1, 12, 5, *args, ws.data_ptr(), need, s) == -1
    assert lib.nm_points_in_mesh(8, 12, -5, *args, ws.data_ptr(), need, s) == -1
    assert lib.nm_points_in_mesh(8, 12, 5, *args, ws.data_ptr(), need - 1, s) == -1
    assert b"workspace" in lib.nm_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all()                                           # nothing was written
    assert lib.nm_points_in_mesh(8, 12, 5, *args, ws.data_ptr(), need, s) == 0
    assert (out.cpu() <= 1).all()


# ------------------------------------------------------------------ 4. the entry point

def _sphere_ply(path, v, t):
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
           "property float z", f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    faces = np.zeros(len(t), dtype=[("k", "u1"), ("i", "<i4", (3,))])
    faces["k"], faces["i"] = 3, t
    path.write_bytes(("\n".join(hdr) + "\n").encode() + np.asarray(v, "<f4").tobytes() + faces.tobytes())


def test_prepare_simulation_data_writes_the_cpu_samplers_particles(tmp_path, monkeypatch):
    from neuma_amd import io as nio, mesh_inside, synth
    from neuma_amd.prepare import prepare_simulation_data
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = synth.make_scene("tiny", override=dict(K=3000, sh=0))
    gm = GaussianModel(0)
    sh = torch.tensor(sc.g_sh)
    gm.set_params(torch.tensor(sc.g_xyz), sh[:, :1].contiguous(), sh[:, 1:].contiguous(), torch.tensor(sc.g_logscale),
                  torch.tensor(sc.g_rot), torch.tensor(sc.g_opacity_logit))
    nio.save_gaussians_ply(gm, tmp_path / "point_cloud.ply")
    xyz = np.asarray(sc.g_xyz, float)
    v, t = uv_sphere(20, 32, r=0.6 * float(np.ptp(xyz, 0).max()) / 2, center=xyz.mean(0))
    _sphere_ply(tmp_path / "mesh.ply", v, t)
    common = dict(kernels_path=tmp_path / "point_cloud.ply", mesh_path=tmp_path / "mesh.ply", mesh_sample_resolution=20, sh_degree=0,
                  device=dev())
    prepare_simulation_data(save_dir=tmp_path / "gpu", **common)
    calls = []

    def cpu_sampler(verts, tris, mode="volumetric", resolution=30, seed=0, device=None):
        calls.append(mode)
        return _cpu().sample_mesh_points(verts, tris, mode, resolution, seed)

    monkeypatch.setattr(mesh_inside, "sample_mesh_points", cpu_sampler)
    prepare_simulation_data(save_dir=tmp_path / "cpu", **common)
    assert calls == ["volumetric"]
    a = (tmp_path / "gpu" / "particles.ply").read_bytes()
    b = (tmp_path / "cpu" / "particles.ply").read_bytes()
    assert a == b and len(nio.load_particles_ply(tmp_path / "gpu" / "particles.ply")) > 1000
    ba = torch.load(tmp_path / "gpu" / "bindings.pt")
    bb = torch.load(tmp_path / "cpu" / "bindings.pt")
    sa = torch.sparse_coo_tensor(ba["bindings_ind"], ba["bindings_val"], ba["bindings_size"]).coalesce()
    sb = torch.sparse_coo_tensor(bb["bindings_ind"], bb["bindings_val"], bb["bindings_size"]).coalesce()
    assert torch.equal(sa.indices(), sb.indices()) and torch.equal(sa.values(), sb.values())
    assert torch.equal(ba["n_particles"], bb["n_particles"])
