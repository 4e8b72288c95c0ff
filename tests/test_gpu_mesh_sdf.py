"""GPU: nm_mesh_distance (csrc/nm_sdf.hip) against the numpy definition neuma_amd/extras/mesh_sdf.py, and build_mesh_field on
the device against its CPU path.

Bound per node: |d_gpu - d_fp64| <= max(4 e32, 1e-6 x the lattice's diagonal), e32 = the largest distance of the definition's
own fp32 evaluation from its fp64 one over the case - the rule the SH-rotation and drawing kernels are held to.  Measured
values: profiles/mesh_sdf_parity_table.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_sdf_cases as cases
from gpu_util import dev, parity
from neuma_amd import _lib as L
from neuma_amd import mesh_sdf
from neuma_amd.extras import mesh_sdf as X

pytestmark = pytest.mark.gpu

MESH_NAMES = ["icosahedron", "sphere320", "torus", "box", "sphere320_bad", "tris257", "single"]


@functools.lru_cache(maxsize=None)
def _reference(name, dims):
    """(verts, tris, origin, spacing, d64, d32) of one case: computed once, shared, never modified"""
    v, t = cases.MESHES[name]()
    origin, h = cases.lattice_for(v, dims)
    d64 = X.mesh_distance(v, t, origin, h, dims, np.float64)
    d32 = X.mesh_distance(v, t, origin, h, dims, np.float32)
    return v, t, origin, h, d64, d32


def _upload(v, t):
    return (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev()),
            torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)).to(dev()))


@pytest.mark.parametrize("dims", cases.LATTICE_DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", MESH_NAMES)
def test_distance_against_the_fp64_definition(name, dims):
    v, t, origin, h, d64, d32 = _reference(name, dims)
    vd, td = _upload(v, t)
    got = mesh_sdf.distance_native(vd, td, origin, h, dims)
    again = mesh_sdf.distance_native(vd, td, origin, h, dims)
    assert got.shape == tuple(dims) and got.dtype == torch.float32
    assert torch.equal(got, again), "two calls differ"
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    e32 = float(np.abs(d32.astype(np.float64) - d64).max())
    diag = float(h) * float(np.linalg.norm(np.asarray(dims) - 1))
    err = float(np.abs(g - d64).max())
    print(f"mesh distance {name} {dims}: e32 {e32:.3e} measured {err:.3e} ratio {err / max(e32, 1e-300):.2f}")
    parity(f"mesh distance {name} {'x'.join(map(str, dims))} ({len(t)} triangles)", "distance (abs)", err, max(4.0 * e32, 1e-6 * diag), noise=e32)
    # the wrapper (its own order of the triangles, its own upload) gives the same bytes: the minimum does not depend on the order
    assert torch.equal(mesh_sdf.mesh_distance(v, t, origin, h, dims, dev()), got)


@pytest.mark.parametrize("dims", cases.LATTICE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_dropped_and_degenerate_triangles_change_nothing(dims):
    """sphere320 with a degenerate triangle just under its surface and a triangle with an out-of-range index: the field of the
    sphere alone, bit for bit (that no node of these lattices is nearer to the degenerate one: tests/test_mesh_sdf_cpu.py)"""
    v0, t0 = cases.sphere320()
    v1, t1 = cases.sphere320_with_bad_triangles()
    origin, h = cases.lattice_for(v0, dims)
    a = mesh_sdf.distance_native(*_upload(v0, t0), origin, h, dims)
    b = mesh_sdf.distance_native(*_upload(v1, t1), origin, h, dims)
    assert torch.equal(a, b)
    # a negative index and one far beyond the vertices, in front of the others
    t2 = np.concatenate([np.array([(-1, 0, 1), (0, 2 ** 31 - 1, 1)], dtype=np.int64), t0])
    assert torch.equal(mesh_sdf.distance_native(*_upload(v0, t2), origin, h, dims), a)


def test_degenerate_triangles_alone_are_segments_and_points():
    v = np.array([(0.2, 0.3, 0.4), (0.5, 0.3, 0.4), (0.8, 0.3, 0.4), (0.5, 0.6, 0.5)], dtype=np.float64)
    t = np.array([(0, 1, 2), (3, 3, 3), (0, 0, 2)], dtype=np.int64)
    origin, h, dims = np.array([0.013, 0.021, 0.007], dtype=np.float32), np.float32(0.0817), (13, 9, 6)
    got = mesh_sdf.distance_native(*_upload(v, t), origin, h, dims).cpu().numpy().astype(np.float64)
    d64, d32 = X.mesh_distance(v, t, origin, h, dims), X.mesh_distance(v, t, origin, h, dims, np.float32)
    e32 = float(np.abs(d32 - d64).max())
    diag = float(h) * float(np.linalg.norm(np.asarray(dims) - 1))
    parity("mesh distance degenerate-only 13x9x6 (3 triangles)", "distance (abs)", float(np.abs(got - d64).max()),
           max(4.0 * e32, 1e-6 * diag), noise=e32)


def test_empty_mesh_is_plus_infinity():
    v, _ = cases.single_triangle()
    for t in (np.zeros((0, 3), dtype=np.int64), np.array([(0, 1, 3), (-1, 0, 1)], dtype=np.int64)):
        got = mesh_sdf.distance_native(*_upload(v, t), np.zeros(3, dtype=np.float32), 0.1, (5, 6, 7))
        assert bool(torch.isinf(got).all()) and bool((got > 0).all())


def test_invalid_sizes_return_minus_one_and_leave_the_output_alone():
    lib = L.lib()
    v, t = _upload(*cases.single_triangle())
    out = torch.full((4, 4, 4), -7.0, device=dev())
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=dev())
    o = (C.c_float * 3)(0, 0, 0)
    for kw in (dict(nt=-1), dict(nv=-1), dict(nt=(1 << 24) + 1), dict(d=(1, 4, 4)), dict(d=(4, 4, 1)), dict(d=(1 << 10, 1 << 10, 1 << 8)),
               dict(h=0.0), dict(h=-0.1), dict(h=float("inf")), dict(h=float("nan")), dict(ws=16)):
        dd = (C.c_int32 * 3)(*kw.get("d", (4, 4, 4)))
        rc = lib.nm_mesh_distance(kw.get("nv", 3), kw.get("nt", 1), v.data_ptr(), t.data_ptr(), o, kw.get("h", 0.1), dd, out.data_ptr(),
                                  ws.data_ptr(), kw.get("ws", ws.numel()), L.stream_ptr(dev()))
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    L.check(lib.nm_mesh_distance(3, 1, v.data_ptr(), t.data_ptr(), o, 0.1, (C.c_int32 * 3)(4, 4, 4), out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), L.stream_ptr(dev())), "nm_mesh_distance")
    assert bool((out >= 0).all())


@pytest.mark.parametrize("name", ["torus", "box"])
def test_build_mesh_field_on_the_device_matches_the_cpu_path(name):
    v, t = cases.MESHES[name]()
    g = mesh_sdf.build_mesh_field(v, t, resolution=21, device=dev())
    c = X.build_mesh_field(v, t, resolution=21)
    assert g.dims == c.dims and g.origin == c.origin and g.spacing == c.spacing
    assert g.phi.is_cuda and g.phi.dtype == torch.float32 and tuple(g.phi.shape) == g.dims
    phi = g.phi.cpu().numpy().astype(np.float64)
    assert np.array_equal(phi < 0, c.phi < 0) and (phi < 0).any()
    d32 = X.mesh_distance(v, t, np.asarray(c.origin, np.float32), np.float32(c.spacing), c.dims, np.float32)
    e32 = float(np.abs(d32 - np.abs(c.phi)).max())
    diag = c.spacing * float(np.linalg.norm(np.asarray(c.dims) - 1))
    parity(f"build_mesh_field {name} resolution 21", "phi (abs)", float(np.abs(phi - c.phi).max()), max(4.0 * e32, 1e-6 * diag), noise=e32)
    with pytest.raises(ValueError, match="not closed"):
        mesh_sdf.build_mesh_field(v, t[:-1], resolution=8, device=dev())
    with pytest.raises(ValueError, match="inverted"):
        mesh_sdf.build_mesh_field(v, t[:, ::-1], resolution=8, device=dev())
