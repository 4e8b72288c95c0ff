"""extras/mesh_sdf.py, the numpy definition of the mesh distance field: the seven Voronoi regions of one triangle against
distances worked out by hand, a triangle soup against a plain pointwise loop, the signed field against points_in_mesh, the
refusals of build_mesh_field, and the conditions the GPU tests rely on (no GPU needed)."""
import math

import numpy as np
import pytest

import mesh_sdf_cases as cases
from neuma_amd.extras import mesh_sdf as X
from neuma_amd.extras import mesh_sampling as ms


# the triangle a = (0,0,0), b = (2,0,0), c = (0,2,0) in the plane z = 0
TRI_V = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)])
TRI_T = np.array([(0, 1, 2)])
REGIONS = [
    # point, distance by hand
    ("face", (0.5, 0.5, 0.75), 0.75),
    ("vertex a", (-3.0, -4.0, 0.0), 5.0),
    ("vertex b", (5.0, -4.0, 0.0), 5.0),                       # b + (3, -4, 0)
    ("vertex c", (-4.0, 5.0, 0.0), 5.0),                       # c + (-4, 3, 0)
    ("edge ab", (1.0, -3.0, 4.0), 5.0),                        # foot (1, 0, 0)
    ("edge ac", (-3.0, 1.0, 4.0), 5.0),                        # foot (0, 1, 0)
    ("edge bc", (2.0, 2.0, 1.0), math.sqrt(2.0 + 1.0)),        # foot (1, 1, 0): in-plane distance sqrt(2), height 1
]


def _dist_points(verts, tris, pts, dtype=np.float64):
    rec = X.triangle_records(verts, tris, dtype)
    return np.sqrt(X.pair_dist2(np.asarray(pts, dtype=dtype), rec).min(axis=1))


@pytest.mark.parametrize("name,p,want", REGIONS, ids=[r[0] for r in REGIONS])
def test_single_triangle_regions_by_hand(name, p, want):
    got = _dist_points(TRI_V, TRI_T, [p])[0]
    assert abs(got - want) <= 1e-14 * max(1.0, want), (name, got, want)
    got32 = _dist_points(TRI_V, TRI_T, [p], np.float32)[0]
    assert got32.dtype == np.float32 and abs(float(got32) - want) <= 1e-6 * max(1.0, want)
    # any cyclic relabelling of the vertices is the same triangle
    for perm in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        assert abs(_dist_points(TRI_V, np.array([perm]), [p])[0] - want) <= 1e-14 * max(1.0, want)


def _closest_on_segment(p, a, b):
    e = b - a
    ee = float(e @ e)
    t = 0.0 if ee == 0.0 else min(max(float((p - a) @ e) / ee, 0.0), 1.0)
    return float(np.linalg.norm(p - (a + t * e)))


def _plain_distance(p, a, b, c):
    """projection onto the plane when the foot is inside (sign of three cross products), else the nearest of the edges"""
    n = np.cross(b - a, c - a)
    nn = float(n @ n)
    if nn > 0.0:
        foot = p - n * (float((p - a) @ n) / nn)
        s = [float(np.cross(q1 - q0, foot - q0) @ n) for q0, q1 in ((a, b), (b, c), (c, a))]
        if min(s) >= 0.0:
            return abs(float((p - a) @ n)) / math.sqrt(nn)
    return min(_closest_on_segment(p, a, b), _closest_on_segment(p, b, c), _closest_on_segment(p, c, a))


def test_triangle_soup_against_a_plain_loop():
    rng = np.random.default_rng(3)
    v = rng.random((40, 3))
    t = rng.integers(0, 40, size=(25, 3))
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    v32 = v.astype(np.float32).astype(np.float64)
    origin, h, dims = np.array([-0.2, -0.1, -0.3], dtype=np.float32), np.float32(0.17), (9, 8, 10)
    got = X.mesh_distance(v, t, origin, h, dims)
    nodes = X.lattice_nodes(origin, h, dims).reshape(-1, 3)
    want = np.array([min(_plain_distance(p, v32[a], v32[b], v32[c]) for a, b, c in t) for p in nodes]).reshape(dims)
    assert np.abs(got - want).max() <= 1e-12
    got32 = X.mesh_distance(v, t, origin, h, dims, dtype=np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 2e-6


def test_degenerate_and_dropped_triangles():
    v = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.5, 0.5, 0.5)])
    pts = [(2.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (4.0, 3.0, 4.0)]
    want = [1.0, 1.0, math.sqrt(1 + 9 + 16)]
    for tri in ((0, 1, 2), (2, 0, 1), (0, 2, 2), (0, 0, 2)):          # collinear; with a zero-length segment
        assert np.allclose(_dist_points(v, np.array([tri]), pts), want, atol=1e-14)
    assert np.allclose(_dist_points(v, np.array([(3, 3, 3)]), [(0.5, 0.5, 1.5)]), [1.0])      # a point
    # out-of-range indices drop the triangle; nothing kept: +inf
    d = X.mesh_distance(v, np.array([(0, 1, 4), (-1, 0, 1)]), np.zeros(3, np.float32), np.float32(0.5), (2, 3, 2))
    assert np.isinf(d).all() and (d > 0).all()
    d = X.mesh_distance(v, np.zeros((0, 3), dtype=np.int64), np.zeros(3, np.float32), np.float32(0.5), (2, 3, 2))
    assert np.isinf(d).all()
    for bad_dims, spacing in (((1, 4, 4), 0.1), ((4, 4, 4), 0.0), ((4, 4, 4), float("nan")), ((1 << 10, 1 << 10, 1 << 8), 0.1)):
        with pytest.raises(ValueError):
            X.mesh_distance(v, np.array([(0, 1, 3)]), np.zeros(3, np.float32), spacing, bad_dims)


def test_bad_triangles_of_the_gpu_case_are_harmless_on_its_lattices():
    """the condition test_gpu_mesh_sdf.py relies on: on both lattices, in fp64 and in the fp32 evaluation, the degenerate and the
    out-of-range triangle leave the field of sphere320 as it is"""
    v0, t0 = cases.sphere320()
    v1, t1 = cases.sphere320_with_bad_triangles()
    assert len(t1) == len(t0) + 2 and len(X.kept_triangles(len(v1), t1)) == len(t0) + 1
    for dims in cases.LATTICE_DIMS:
        origin, h = cases.lattice_for(v0, dims)
        for dt in (np.float64, np.float32):
            assert np.array_equal(X.mesh_distance(v0, t0, origin, h, dims, dt), X.mesh_distance(v1, t1, origin, h, dims, dt))


@pytest.mark.parametrize("name", ["icosahedron", "torus", "box"])
def test_build_mesh_field_sign_is_points_in_mesh(name):
    v, t = cases.MESHES[name]()
    f = X.build_mesh_field(v, t, resolution=13, margin_cells=2)      # (odd: no node lands on a vertex, where phi = 0)
    assert f.phi.shape == f.dims and min(f.dims) >= 5
    v32 = v.astype(np.float32).astype(np.float64)
    lo, hi = v32.min(0), v32.max(0)
    o = np.asarray(f.origin)
    assert np.allclose(o, lo - 2 * f.spacing, atol=1e-6) and (o + (np.asarray(f.dims) - 1) * f.spacing >= hi + 2 * f.spacing - 1e-6).all()
    assert abs(f.spacing - (hi - lo).max() / 13) <= 1e-7
    nodes = X.lattice_nodes(f.origin, f.spacing, f.dims).reshape(-1, 3)
    inside = ms.points_in_mesh(nodes, v32, t).reshape(f.dims)
    assert inside.any() and not inside.all()
    assert np.array_equal(f.phi < 0, inside)
    assert np.array_equal(np.abs(f.phi), X.mesh_distance(v, t, np.asarray(f.origin, np.float32), np.float32(f.spacing), f.dims))
    # the margin is outside
    assert (f.phi[0] > 0).all() and (f.phi[-1] > 0).all() and (f.phi[:, 0] > 0).all() and (f.phi[:, :, -1] > 0).all()
    f2 = X.build_mesh_field(v, t, spacing=0.05, margin_cells=1)
    assert abs(f2.spacing - np.float32(0.05)) < 1e-9


def test_build_mesh_field_refuses_open_and_inverted_meshes():
    v, t = cases.MESHES["box"]()
    with pytest.raises(ValueError, match=r"not closed: 3 edges"):
        X.build_mesh_field(v, t[:-1], resolution=8)
    with pytest.raises(ValueError, match="inverted"):
        X.build_mesh_field(v, t[:, ::-1], resolution=8)
    assert X.open_edges(len(v), t) == 0
    # an out-of-range triangle is dropped before the check: the mesh stays closed
    f = X.build_mesh_field(v, np.concatenate([t, [(0, 1, 99)]]), resolution=8)
    assert (f.phi < 0).any()


def test_gpu_wrapper_takes_the_cpu_path_on_request():
    from neuma_amd import mesh_sdf
    v, t = cases.MESHES["box"]()
    a, b = mesh_sdf.build_mesh_field(v, t, resolution=8, device="cpu"), X.build_mesh_field(v, t, resolution=8)
    assert isinstance(a, mesh_sdf.MeshField) and np.array_equal(a.phi, b.phi) and a.dims == b.dims


def test_cull_order_is_a_fixed_permutation_and_the_field_ignores_it():
    v, t = cases.MESHES["torus"]()
    o = X.cull_order(len(t))
    assert sorted(o.tolist()) == list(range(len(t))) and np.array_equal(o, X.cull_order(len(t))) and len(X.cull_order(0)) == 0
    origin, h = cases.lattice_for(v, (13, 9, 6))
    assert np.array_equal(X.mesh_distance(v, t, origin, h, (13, 9, 6), np.float32), X.mesh_distance(v, t[o], origin, h, (13, 9, 6), np.float32))


def test_abi_rejects_invalid_sizes_on_the_host():
    """nm_mesh_distance validates before any device work: callable without a GPU"""
    import ctypes as C
    from neuma_amd import _lib as L
    lib = L.lib()
    o, d = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    assert lib.nm_mesh_distance_workspace(10, 64) >= 640 and lib.nm_mesh_distance_workspace(-1, 64) == 0
    assert lib.nm_mesh_distance_workspace((1 << 24) + 1, 64) == 0 and lib.nm_mesh_distance_workspace(1, (1 << 27) + 1) == 0
    fake = 256      # never dereferenced: every call below fails its validation
    for kw in (dict(nt=-1), dict(nv=-1), dict(nt=(1 << 24) + 1), dict(d=(1, 4, 4)), dict(d=(1 << 10, 1 << 10, 1 << 8)),
               dict(h=0.0), dict(h=float("inf")), dict(h=float("nan")), dict(ws=16)):
        dd = (C.c_int32 * 3)(*kw.get("d", (4, 4, 4)))
        rc = lib.nm_mesh_distance(kw.get("nv", 3), kw.get("nt", 1), fake, fake, o, kw.get("h", 0.1), dd, fake, fake, kw.get("ws", 1 << 20), None)
        assert rc == -1, kw
        assert lib.nm_last_error()
