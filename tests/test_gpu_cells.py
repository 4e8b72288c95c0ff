"""GPU: what csrc/nm_cells.h shares among nm_bindbuild, nm_fill, nm_nn and nm_mesh (the cell fit, nm_cell, k_nm_segment_starts,
the carved rocPRIM scan / pair sort), at the smallest shapes where those pieces can go wrong: empty and one-element inputs,
everything in the first or the last segment, budgets of one and two cells, one row / one column of cells, boxes of
different shapes in one call.  Every case is held to the yardstick its neighbour uses: extras/binding_cpu.py (integers exact),
extras/gaussian_fill.py (check_field of test_gpu_gaussian_fill.py; an all-zero field exact), the fp64 brute force of
knn_ref.py and the fixed-order mean of test_gpu_particle_metrics.py (bit for bit), extras/mesh_sampling.py (mask for mask).

Not repeated here: a cloud of 4 points, a planar cloud (one zero-extent axis) and a cloud of coincident points (three) are
CLOUDS["n4_k3"], ["plane200"] and ["coincident64"] of test_gpu_knn.py; a mesh of no triangles is
test_gpu_mesh_inside.py::test_edge_cases_and_errors."""
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest
import torch

from gpu_util import dev, measured
from knn_ref import knn_brute

pytestmark = pytest.mark.gpu

THR = 7.814727903251179          # chi2.ppf(0.95, 3)


# ------------------------------------------------------------------ nm_bind_build on a lattice of the test's choosing

LATTICE = (np.zeros(3, np.float32), 1.0, np.array([3, 4, 5], np.int32))      # cells [0, 3) x [0, 4) x [0, 5), edge 1


def _gaussians():
    """three whose boxes cover the whole lattice (sigma 6 .. 12 against a lattice 5 long), one a cell wide in the last cell, one
    in an empty middle cell"""
    means = np.array([[1.5, 2.0, 2.5], [0.2, 0.3, 0.1], [2.9, 3.8, 4.9], [2.5, 3.5, 4.5], [1.5, 1.5, 2.5]], np.float32)
    cov6 = np.array([[100, 0, 0, 100, 0, 100], [64, 5, -3, 81, 7, 36], [49, -4, 2, 144, 6, 64], [0.04, 0, 0, 0.05, 0.01, 0.04],
                     [0.01, 0, 0, 0.01, 0, 0.01]], np.float32)
    return means, cov6


def _particles(name):
    r = np.random.default_rng(5)
    first, last = r.uniform(0.05, 0.95, (5, 3)), r.uniform(0.05, 0.95, (5, 3)) + np.array([2.0, 3.0, 4.0])
    return {"none": np.zeros((0, 3)), "one": last[:1], "all_in_cell_0": first, "all_in_the_last_cell": last,
            "first_and_last_cell_only": np.concatenate([first[:3], last[:4]])}[name].astype(np.float32)


def _bind_native(means, cov6, x, maxp):
    from neuma_amd import _lib as L
    lib, d = L.lib(), dev()
    origin, h, dims = LATTICE
    m, c, xx = (torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in (means, cov6, x))
    K, N = len(means), len(x)
    ws_bytes = int(lib.nm_bind_build_workspace(N, int(np.prod(dims))))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=d)
    counts = torch.full((K,), -7, dtype=torch.int32, device=d)
    inside = torch.full((K,), -7, dtype=torch.int32, device=d)
    cols = torch.full((K, maxp), -7, dtype=torch.int32, device=d)
    pv = torch.full((K, maxp), -7.0, dtype=torch.float32, device=d)
    L.check(lib.nm_bind_build(K, N, L.ptr(m), L.ptr(c), L.ptr(xx) if N else None, (C.c_float * 3)(*origin.tolist()), float(h),
                              (C.c_int32 * 3)(*dims.tolist()), THR, maxp, L.ptr(counts), L.ptr(inside), L.ptr(cols), L.ptr(pv),
                              L.ptr(ws), ws_bytes, L.stream_ptr(d)), "nm_bind_build")
    return tuple(t.cpu().numpy() for t in (counts, inside, cols, pv))


@pytest.mark.parametrize("name", ["none", "one", "all_in_cell_0", "all_in_the_last_cell", "first_and_last_cell_only"])
def test_bind_build_with_empty_first_and_last_segments(name):
    from neuma_amd.extras import binding_cpu
    means, cov6 = _gaussians()
    x = _particles(name)
    maxp = 4                                             # fewer than the 5 .. 7 particles the covering Gaussians hold: the clip runs
    want = binding_cpu.build_bindings(means, cov6, x, THR, maxp)
    got = _bind_native(means, cov6, x, maxp)
    if len(x) >= 5:
        assert (want[1][:3] == len(x)).all() and want[1][4] == 0 and (want[0][:3] == maxp).all()
    for g, w, what in zip(got[:3], want[:3], ("counts", "n_inside", "cols")):
        assert g.dtype == w.dtype and measured(int((g != w).sum()), f"{name}: {what} differing from binding_cpu") <= 0
    assert np.allclose(got[3], want[3], rtol=5e-5, atol=1e-6)      # (the bound of test_gpu_binding.py; fp32, another fma order)


# ------------------------------------------------------------------ Gaussian fill on a 5 x 6 x 7 lattice (2 x 2 x 2 blocks)

FILL_LATTICE = (np.zeros(3), 1.0, np.array([5, 6, 7], np.int32))


def _fill(mu, cv, op):
    from neuma_amd import gaussian_fill as gpu
    from neuma_amd.extras import gaussian_fill as cpu
    origin, h, dims = FILL_LATTICE
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    sc = SimpleNamespace()
    sc.f64, sc.skipped = cpu.density_field(mu, cv, op, origin, h, dims, 9.0)
    sc.f32, _ = cpu.density_field(mu, cv, op, origin, h, dims, 9.0, dtype=np.float32)
    sc.gpu_field, sc.gpu_skipped = gpu.density_field(up(mu), up(cv), up(op), origin, h, dims, 9.0)
    return sc


def test_fill_gaussian_in_the_last_partial_block_only():
    from neuma_amd.extras import gaussian_fill as cpu
    from test_gpu_gaussian_fill import check_field
    mu, cv, op = np.array([[4.5, 4.95, 5.5]], np.float32), np.array([[0.01, 0, 0, 0.04, 0, 0.01]], np.float32), np.array([0.8], np.float32)
    b0, b1 = cpu.gaussian_blocks(mu, cv, *FILL_LATTICE)
    assert b0.tolist() == [[1, 1, 1]] and b1.tolist() == [[1, 1, 1]]      # the block of cells x 4, y 4..5, z 4..6: partial on every axis
    sc = _fill(mu, cv, op)
    check_field(sc, float(sc.f64.max()))
    g = sc.gpu_field.cpu().numpy().reshape(5, 6, 7)
    assert g[4, 4:, 4:].max() > 0 and np.count_nonzero(g) == np.count_nonzero(g[4, 4:, 4:])      # the seven other blocks: zeros


def test_fill_without_any_pair():
    flat = np.array([[0.01, 0, 0, 0.01, 0, 0.0], [0.01, 0.02, 0, 0.01, 0, 0.01]], np.float32)      # det <= 0: no block each
    sc = _fill(np.full((2, 3), 2.5, np.float32), flat, np.ones(2, np.float32))
    assert sc.skipped == 2 and sc.gpu_skipped == 2 and not sc.f64.any()
    g = sc.gpu_field.cpu().numpy()
    assert g.shape == (5 * 6 * 7,) and measured(np.count_nonzero(g.view(np.uint32)), "non-zero words of an empty field") <= 0


# ------------------------------------------------------------------ nm_knn / nm_chamfer on the smallest grids

def _rand(shape, seed):
    return torch.rand(*shape, 3, generator=torch.Generator().manual_seed(seed)).float()


def _small_clouds():
    """name -> (a (B, N, 3), b (B, M, 3), k)"""
    c = {f"cloud_of_{n}": (_rand((1, n), 20 + n), _rand((1, n), 30 + n), n) for n in (1, 2, 3)}      # cell budgets 1, 1, 2
    line = torch.zeros(1, 17, 3)
    line[0, :, 0] = torch.rand(17, generator=torch.Generator().manual_seed(40)) * 4 - 1
    line[0, :, 1:] = torch.tensor([0.3, -0.7])
    c["collinear17"] = (line, line + torch.tensor([0.01, 0.0, 0.0]), 3)                               # two zero-extent axes
    a, b = _rand((3, 40), 41), _rand((3, 33), 42)
    for t in (a, b):                                                                                  # item 0 stays a cube
        t[1] *= torch.tensor([1.0, 1.0, 1e-3])                                                        # a plate
        t[2] *= torch.tensor([1e-4, 50.0, 1e-4])                                                      # a rod
    c["three_shapes_in_one_call"] = (a, b + 0.25, 4)
    return c


SMALL = _small_clouds()
_SMALL_REF = {}


def _small_ref(name):
    """per item ((idx, d2) of a in b, k best; of b in a, the nearest), once"""
    if name not in _SMALL_REF:
        a, b, k = SMALL[name]
        _SMALL_REF[name] = [(knn_brute(a[i], b[i], k), knn_brute(b[i], a[i], 1)) for i in range(a.shape[0])]
    return _SMALL_REF[name]


def _bits_differ(x, y):
    return int((x.contiguous().view(torch.int64) != y.contiguous().view(torch.int64)).sum())


@pytest.mark.parametrize("name", sorted(SMALL))
def test_knn_on_the_smallest_grids(name):
    from neuma_amd.particle_metrics import k_nearest_neighbors
    a, b, k = SMALL[name]
    idx, d2 = k_nearest_neighbors(a.to(dev()), b.to(dev()), k)
    for i, ((ridx, rd2), _) in enumerate(_small_ref(name)):
        assert measured(int((idx[i].cpu() != ridx).sum()), f"{name}[{i}]: index mismatches") <= 0
        assert measured(_bits_differ(d2[i].cpu(), rd2), f"{name}[{i}]: distance bit mismatches") <= 0


@pytest.mark.parametrize("name", sorted(SMALL))
def test_chamfer_on_the_smallest_grids(name):
    from neuma_amd.particle_metrics import chamfer_native
    from test_gpu_particle_metrics import _fixed_order_mean
    a, b, _ = SMALL[name]
    cd12, cd21, i12, i21 = (t.cpu() for t in chamfer_native(a.to(dev()), b.to(dev())))
    for i, ((ridx, rd2), (sidx, sd2)) in enumerate(_small_ref(name)):
        assert measured(int((i12[i] != ridx[:, 0]).sum()) + int((i21[i] != sidx[:, 0]).sum()), f"{name}[{i}]: index mismatches") <= 0
        want = torch.tensor([_fixed_order_mean(rd2[:, 0].numpy()), _fixed_order_mean(sd2[:, 0].numpy())], dtype=torch.float64)
        assert measured(_bits_differ(torch.stack([cd12[i], cd21[i]]), want), f"{name}[{i}]: mean bit mismatches") <= 0


# ------------------------------------------------------------------ nm_points_in_mesh: one cell, one row, one column of cells

def _tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.0, 0.1], [0.3, 0.4, 1.0]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)      # 4 triangles: a budget of one cell


def _strip(transpose):
    """64 triangles between y = 0 and y = 0.001 from x = 0 to x = 1000, rising in z: 16 x 1 cells (1 x 16 transposed)"""
    x = np.linspace(0.0, 1000.0, 33)
    v = np.concatenate([np.stack([x, np.zeros(33), 1.0 + x / 1000.0], 1), np.stack([x, np.full(33, 1e-3), 1.5 + x / 1000.0], 1)])
    i = np.arange(32)
    t = np.concatenate([np.stack([i, i + 1, i + 33], 1), np.stack([i + 1, i + 34, i + 33], 1)]).astype(np.int32)
    return (v[:, [1, 0, 2]] if transpose else v), t


@pytest.mark.parametrize("name", ["tetrahedron", "strip", "strip_transposed"])
def test_points_in_mesh_with_one_cell_one_row_one_column(name):
    from neuma_amd import mesh_inside
    from neuma_amd.extras import mesh_sampling
    v, t = _tetrahedron() if name == "tetrahedron" else _strip(name == "strip_transposed")
    r = np.random.default_rng(7)
    lo, hi = v.min(0), v.max(0)
    inside_box = r.uniform(lo, hi, (400, 3)) * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0]) * r.uniform(-0.5, 3.0, (400, 1))
    around = r.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (200, 3))
    pts = np.concatenate([inside_box, around, v[t[:, 0]], v.mean(0, keepdims=True)])      # vertices themselves included
    want = mesh_sampling.points_in_mesh(pts, v, t)
    got = mesh_inside.points_in_mesh(pts, v, t, dev())
    assert 0 < want.sum() < len(want)
    assert got.dtype == bool and measured(int((got != want).sum()), f"{name}: masks differing from the CPU test") <= 0
