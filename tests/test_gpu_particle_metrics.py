"""GPU: the exact nearest-neighbour search and Chamfer distance of csrc/nm_nn.hip (nm_chamfer, nm_nearest_neighbors) through
neuma_amd.particle_metrics - against the reference's own metrics.py output (tests/golden/chamfer, fp32), against scipy's cKDTree
in fp64 at 10^5 and 10^6 points, on degenerate inputs, for reproducibility and for the gradient - and
`python -m neuma_amd.particle_evaluation` end to end."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from gpu_util import abs_max, dev, measured, rel_max

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLD))
import chamfer_inputs as CI  # noqa: E402


def _pm():
    from neuma_amd import particle_metrics
    return particle_metrics


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _d2(q, t, idx):
    """fp64 squared distance of every query to the target `idx` (numpy, summed x, y, z in order)"""
    q, t = q.astype(np.float64), t.astype(np.float64)
    return ((q - t[idx]) ** 2).sum(-1)


def _check_against_kdtree(q, t, idx, d2=None, mean=None):
    """idx (N,) / d2 (N,) / mean of one direction against cKDTree in fp64: indices equal, or else the two candidates' fp64
    distances equal (an exact tie); the mean to 1e-12 relative."""
    _, ref = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=1)
    dr = _d2(q, t, ref)
    do = _d2(q, t, idx)
    diff = idx != ref
    assert measured(np.abs(do - dr).max() / max(dr.max(), 1e-300), "nn d2 rel (differing indices are ties)") <= 1e-15
    assert measured(diff.mean(), "fraction of indices that differ from cKDTree (ties)") <= 0.01
    if d2 is not None:
        assert rel_max(torch.from_numpy(d2), torch.from_numpy(do)) < 1e-15
    if mean is not None:
        assert measured(abs(mean - dr.mean()) / dr.mean(), "chamfer mean rel vs cKDTree fp64") < 1e-12


# ------------------------------------------------------------------ the reference's own output


@pytest.mark.parametrize("name", sorted(CI.KDTREE_CASES))
def test_matches_the_reference_fixtures(name):
    pm = _pm()
    a, b = CI.KDTREE_CASES[name]()
    g = np.load(GOLD / "chamfer" / f"{name}.npz")
    c1, c2, i12, i21 = pm.chamfer_distance(_g(a), _g(b), give_id=True)
    assert c1.dtype == torch.float32 and i12.dtype == torch.int64 and i12.shape == a.shape[:2] and i21.shape == b.shape[:2]
    assert rel_max(c1, torch.from_numpy(g["chamfer1"])) < 2e-6
    assert rel_max(c2, torch.from_numpy(g["chamfer2"])) < 2e-6
    assert rel_max(pm.chamfer_distance(_g(a), _g(b)), torch.from_numpy(g["chamfer"])) < 2e-6
    for q, t, mine, ref in ((a, b, i12, g["idx12"]), (b, a, i21, g["idx21"])):
        mine = mine.cpu().numpy()
        for k in range(q.shape[0]):
            d = ((q[k][:, None, :].astype(np.float64) - t[k][None].astype(np.float64)) ** 2).sum(-1)
            unique = (d == d.min(1, keepdims=True)).sum(1) == 1
            assert measured((mine[k][unique] != ref[k][unique]).sum(), "index mismatches where the neighbour is unique") <= 0
            assert np.array_equal(d[np.arange(len(d)), mine[k]], d.min(1))         # ties: still a nearest neighbour


def test_matches_the_naive_fixture():
    pm = _pm()
    a, b = CI.naive()
    g = np.load(GOLD / "chamfer" / "naive.npz")
    assert rel_max(pm.chamfer_distance_naive(_g(a), _g(b)), torch.from_numpy(g["chamfer"])) < 2e-6
    assert rel_max(pm.chamfer_distance(_g(a), _g(b), use_kdtree=False), torch.from_numpy(g["chamfer"])) < 2e-6
    with pytest.raises(AssertionError):
        pm.chamfer_distance_naive(_g(a), _g(b[:, :300]))


# ------------------------------------------------------------------ cKDTree in fp64 at size


@pytest.mark.parametrize("n,m", [(100_000, 100_000), (1_000_000, 800_000)])
def test_against_ckdtree_at_size(n, m):
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(11))
    a = CI._lattice_ball(n, 128, r)[None].astype(np.float32)
    b = (r.uniform(0.2, 0.8, (1, m, 3)) + 0.01 * r.normal(size=(1, m, 3))).astype(np.float32)
    cd12, cd21, i12, i21 = pm.chamfer_native(_g(a), _g(b))
    _check_against_kdtree(a[0], b[0], i12[0].cpu().numpy(), mean=float(cd12[0]))
    _check_against_kdtree(b[0], a[0], i21[0].cpu().numpy(), mean=float(cd21[0]))


def test_one_chamfer_call_equals_two_nearest_neighbor_calls():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(12))
    a, b = _g(r.uniform(0, 1, (3, 5000, 3)).astype(np.float32)), _g(r.normal(0.5, 0.3, (3, 7000, 3)).astype(np.float32))
    cd12, cd21, i12, i21 = pm.chamfer_native(a, b)
    j12, d12 = pm.nearest_neighbors(a, b)
    j21, d21 = pm.nearest_neighbors(b, a)
    assert measured(int((i12 != j12).sum()) + int((i21 != j21).sum()), "index differences between the two entry points") <= 0
    assert rel_max(cd12, d12.mean(1)) < 1e-14
    assert rel_max(cd21, d21.mean(1)) < 1e-14
    for k in range(3):
        _check_against_kdtree(a[k].cpu().numpy(), b[k].cpu().numpy(), j12[k].cpu().numpy(), d2=d12[k].cpu().numpy())


def test_two_calls_give_identical_bits():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(13))
    a, b = _g(r.uniform(0, 1, (4, 20000, 3)).astype(np.float32)), _g(r.uniform(0, 1, (4, 15000, 3)).astype(np.float32))
    x = pm.chamfer_native(a, b)
    y = pm.chamfer_native(a, b)
    for u, v in zip(x, y):
        assert measured(int((u.view(torch.int64) != v.view(torch.int64)).sum()), "bit differences between two calls") <= 0


def _xor_tree(v):
    """the wave reduce of csrc/nm_reduce.h over the last axis (64 lanes): v = v + v[lane ^ o], o = 32 .. 1"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def _fixed_order_mean(d2):
    """k_nn_mean_part + k_nn_mean_finish of csrc/nm_nn.hip on one item's d2 (N,), one IEEE fp64 operation at a time"""
    n = len(d2)
    gm = min(max(-(-n // 4096), 1), 64)
    stride = gm * 256
    rounds = -(-n // stride)
    x = np.zeros(rounds * stride)                 # (a thread past the end adds nothing; d2 >= 0, so + 0.0 changes no bit)
    x[:n] = d2
    acc = np.zeros(stride)                        # thread t of block b sums i = b * 256 + t, + gm * 256, ... in turn
    for k in range(rounds):
        acc = acc + x[k * stride:(k + 1) * stride]
    w = _xor_tree(acc.reshape(gm, 4, 64))[..., 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]      # the waves left to right
    lanes = np.zeros(64)                          # finish: lane j sums partials j, j + 64, ... (gm <= 64: at most one)
    lanes[:gm] = part
    return _xor_tree(lanes)[0] / np.float64(n)


@pytest.mark.parametrize("n", [1, 255, 257, 4097, 64 * 4096 + 3])
def test_chamfer_means_are_the_documented_fixed_order_sum(n):
    """n: one lane; fewer than 4 full waves; a second wave; two workgroups per item; the cap of 64 with the strided loop
    running twice."""
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(26))
    a, b = _g(r.uniform(0, 1, (2, n, 3)).astype(np.float32)), _g(r.normal(0.5, 0.3, (2, 1000, 3)).astype(np.float32))
    cd12, cd21, _, _ = pm.chamfer_native(a, b)
    assert cd12.dtype == torch.float64 and cd21.dtype == torch.float64
    for cd, (q, t) in ((cd12, (a, b)), (cd21, (b, a))):
        d2 = pm.nearest_neighbors(q, t)[1].cpu().numpy()
        assert d2.dtype == np.float64 and d2.shape == q.shape[:2]
        want = np.array([_fixed_order_mean(d2[k]) for k in range(2)])
        assert measured(int((cd.cpu().numpy().view(np.int64) != want.view(np.int64)).sum()),
                        "bit differences between the kernel's mean and the emulated fixed-order sum") <= 0


# ------------------------------------------------------------------ degenerate inputs


def _both_directions_vs_kdtree(a, b):
    pm = _pm()
    cd12, cd21, i12, i21 = pm.chamfer_native(_g(a), _g(b))
    for k in range(a.shape[0]):
        _check_against_kdtree(a[k], b[k], i12[k].cpu().numpy(), mean=float(cd12[k]))
        _check_against_kdtree(b[k], a[k], i21[k].cpu().numpy(), mean=float(cd21[k]))
    return cd12, cd21, i12, i21


def test_targets_all_one_point():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(14))
    q = r.uniform(0, 1, (1, 3000, 3)).astype(np.float32)
    t = np.full((1, 1000, 3), 0.3, dtype=np.float32)
    idx, d2 = pm.nearest_neighbors(_g(q), _g(t))
    assert measured(int(idx.abs().sum()), "index sum (all ties -> index 0)") <= 0
    assert rel_max(d2[0], torch.from_numpy(_d2(q[0], t[0], np.zeros(3000, dtype=np.int64)))) < 1e-15
    _both_directions_vs_kdtree(q, t)


def test_flat_cloud():
    r = np.random.Generator(np.random.PCG64(15))
    t = r.uniform(0, 1, (1, 20000, 3)).astype(np.float32)
    t[..., 2] = 0.5
    q = r.uniform(0, 1, (1, 10000, 3)).astype(np.float32)
    _both_directions_vs_kdtree(q, t)
    t2 = t.copy()
    t2[..., 1] = -2.0                                                          # a line: two axes of zero extent
    _both_directions_vs_kdtree(q, t2)


def test_queries_far_outside_the_box():
    r = np.random.Generator(np.random.PCG64(16))
    t = r.uniform(0, 1, (1, 20000, 3)).astype(np.float32)
    q = r.uniform(0, 1, (1, 2000, 3)).astype(np.float32)
    q[0, :1000] += np.array([10.0, 0.0, 0.0], dtype=np.float32)
    q[0, 1000:] += np.array([-10.0, 10.0, -10.0], dtype=np.float32)
    _both_directions_vs_kdtree(q, t)


def test_clusters_in_a_large_box():
    r = np.random.Generator(np.random.PCG64(17))
    a = np.concatenate([r.normal(0, 0.01, (10000, 3)), r.normal(5, 0.01, (10000, 3))])[None].astype(np.float32)
    b = np.concatenate([r.normal(0, 0.01, (8000, 3)), r.normal(5, 0.01, (9000, 3))])[None].astype(np.float32)
    _both_directions_vs_kdtree(a, b)


def test_a_nan_row_makes_only_its_item_nan():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(18))
    a, b = r.uniform(0, 1, (3, 4000, 3)).astype(np.float32), r.uniform(0, 1, (3, 3000, 3)).astype(np.float32)
    clean = pm.chamfer_native(_g(a), _g(b))
    a[1, 123, 1] = np.nan
    cd12, cd21, _, _ = pm.chamfer_native(_g(a), _g(b))
    assert bool(torch.isnan(cd12[1])) and bool(torch.isnan(cd21[1]))
    for k in (0, 2):
        assert abs_max(cd12[k], clean[0][k]) == 0.0 and abs_max(cd21[k], clean[1][k]) == 0.0
    b2 = b.copy()
    b2[2, 7, 0] = np.inf
    cd12, cd21, _, _ = pm.chamfer_native(_g(a), _g(b2))
    assert bool(torch.isnan(cd12[2])) and bool(torch.isnan(cd21[2])) and bool(torch.isfinite(cd12[0]))


@pytest.mark.parametrize("B", [1, 16])
def test_batch_sizes(B):
    r = np.random.Generator(np.random.PCG64(19 + B))
    a = r.uniform(0, 1, (B, 3000, 3)).astype(np.float32) * r.uniform(0.5, 2.0, (B, 1, 1)).astype(np.float32)
    b = r.normal(0.5, 0.2, (B, 2500, 3)).astype(np.float32)
    _both_directions_vs_kdtree(a, b)


def test_single_point_clouds():
    r = np.random.Generator(np.random.PCG64(21))
    a, b = r.uniform(0, 1, (2, 1, 3)).astype(np.float32), r.uniform(0, 1, (2, 500, 3)).astype(np.float32)
    _both_directions_vs_kdtree(a, b)
    _both_directions_vs_kdtree(b, a)
    _both_directions_vs_kdtree(a, a[:, :, ::-1].copy())


# ------------------------------------------------------------------ errors


def test_rejected_inputs():
    from neuma_amd import _lib as L
    pm = _pm()
    a = torch.rand(1, 10, 3, device=dev())
    with pytest.raises(ValueError):
        pm.chamfer_distance(a, torch.empty(1, 0, 3, device=dev()))
    with pytest.raises(ValueError):
        pm.chamfer_distance(torch.empty(1, 0, 3, device=dev()), a)
    with pytest.raises(L.NeumaHipError):
        pm.chamfer_distance(a.cpu(), a.cpu())
    with pytest.raises(L.NeumaHipError):
        pm.chamfer_distance(a, a.cpu())
    with pytest.raises(NotImplementedError):
        pm.get_nearest_neighbors_indices_batch(np.zeros((1, 4, 3)), np.zeros((1, 4, 3)), k=2)
    lib = L.lib()
    d = torch.empty(4, dtype=torch.float64, device=dev())
    ws_bytes = int(lib.nm_chamfer_workspace(1, 10, 10))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    p = a.data_ptr()
    args = (p, p, d.data_ptr(), d.data_ptr(), None, None, ws.data_ptr())
    assert lib.nm_chamfer(0, 10, 10, *args, ws_bytes, None) == -1
    assert lib.nm_chamfer(1, 0, 10, *args, ws_bytes, None) == -1
    assert lib.nm_chamfer(1, 10, 10, *args, ws_bytes - 1, None) == -1 and b"workspace" in lib.nm_last_error()
    assert lib.nm_nn_workspace(0, 1, 1) == 0 and lib.nm_chamfer_workspace(1, 1, 0) == 0
    assert lib.nm_nearest_neighbors(1, 10, 0, p, p, d.data_ptr(), None, ws.data_ptr(), ws_bytes, None) == -1


# ------------------------------------------------------------------ numpy interface, dtype, gradient


def test_get_nearest_neighbors_indices_batch_matches_ckdtree():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(22))
    src, tgt = r.uniform(0, 1, (2, 3000, 3)).astype(np.float32), r.uniform(0, 1, (2, 4000, 3)).astype(np.float32)
    idx, dist = pm.get_nearest_neighbors_indices_batch(src, tgt)
    assert isinstance(idx, list) and len(idx) == 2 and idx[0].dtype == np.int64 and dist[0].dtype == np.float64
    for k in range(2):
        dr, ir = cKDTree(tgt[k]).query(src[k], k=1)
        assert measured((idx[k] != ir).sum(), "index differences vs cKDTree") <= 0
        assert rel_max(torch.from_numpy(dist[k]), torch.from_numpy(dr)) < 1e-15


def test_fp64_inputs_come_back_fp64():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(23))
    a, b = _g(r.uniform(0, 1, (2, 800, 3))), _g(r.uniform(0, 1, (2, 900, 3)))
    cd = pm.chamfer_distance(a, b)
    assert cd.dtype == torch.float64 and cd.shape == (2,)
    c1, c2, i12, i21 = pm.chamfer_distance(a, b, give_id=True)
    ref1 = ((a - torch.gather(b, 1, i12.unsqueeze(-1).expand(-1, -1, 3))) ** 2).sum(2).mean(1)
    assert rel_max(c1, ref1) < 1e-15 and rel_max(cd, c1 + c2) < 1e-15


def test_gradient_matches_fp64_autograd_of_the_gather_formula():
    pm = _pm()
    r = np.random.Generator(np.random.PCG64(24))
    a0, b0 = r.uniform(0, 1, (2, 700, 3)), r.uniform(0, 1, (2, 500, 3))
    a, b = _g(a0).requires_grad_(), _g(b0).requires_grad_()
    c1, c2, i12, i21 = pm.chamfer_distance(a, b, give_id=True)
    w = torch.tensor([0.7, -1.3], dtype=torch.float64, device=dev())
    ((c1 + 2.0 * c2) * w).sum().backward()
    ac, bc = torch.from_numpy(a0).requires_grad_(), torch.from_numpy(b0).requires_grad_()
    j12, j21 = i12.cpu(), i21.cpu()
    r1 = (ac - torch.gather(bc, 1, j12.view(2, -1, 1).expand_as(ac))).pow(2).sum(2).mean(1)    # metrics.py:69-79
    r2 = (bc - torch.gather(ac, 1, j21.view(2, -1, 1).expand_as(bc))).pow(2).sum(2).mean(1)
    ((r1 + 2.0 * r2) * w.cpu()).sum().backward()
    assert rel_max(a.grad, ac.grad) < 1e-13
    assert rel_max(b.grad, bc.grad) < 1e-13
    af, bf = _g(a0.astype(np.float32)).requires_grad_(), _g(b0.astype(np.float32)).requires_grad_()
    pm.chamfer_distance(af, bf).sum().backward()
    assert af.grad.dtype == torch.float32 and bool(torch.isfinite(af.grad).all()) and bool(torch.isfinite(bf.grad).all())


# ------------------------------------------------------------------ entry point


def test_entry_point_end_to_end(tmp_path):
    from neuma_amd.io import save_particles_ply
    r = np.random.Generator(np.random.PCG64(25))
    pred, gt = tmp_path / "states_run", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    sizes = {0: (3000, 2500), 2: (3000, 2500), 4: (1200, 2500), 6: (3000, 2500)}
    clouds = {}
    for i, (n, m) in sizes.items():
        p = r.uniform(0, 1, (n, 3)).astype(np.float32)
        g = (r.uniform(0, 1, (m, 3)) * 1.1).astype(np.float32)
        save_particles_ply(pred / f"{i:03d}.ply", p)
        save_particles_ply(gt / f"{i:03d}.ply", g)
        clouds[i] = (p, g)
    env = dict(os.environ)
    proc = subprocess.run([sys.executable, "-m", "neuma_amd.particle_evaluation", "-p", str(pred), "-g", str(gt), "-s", "0",
                           "-k", "2", "-n", "3"], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    lines = (tmp_path / "states_run_chamfer.txt").read_text().splitlines()
    rows = [ln.split() for ln in lines[1:]]
    assert [x[0] for x in rows] == ["000", "002", "004", "006", "mean"]
    got = np.array([[float(v) for v in x[1:]] for x in rows])
    ref = []
    for i in (0, 2, 4, 6):
        p, g = clouds[i]
        d12 = cKDTree(g.astype(np.float64)).query(p.astype(np.float64))[0] ** 2
        d21 = cKDTree(p.astype(np.float64)).query(g.astype(np.float64))[0] ** 2
        ref.append([d12.mean() + d21.mean(), d12.mean(), d21.mean()])
    ref = np.array(ref)
    assert rel_max(torch.from_numpy(got[:4]), torch.from_numpy(ref)) < 2e-6
    assert rel_max(torch.from_numpy(got[4]), torch.from_numpy(ref.mean(0))) < 2e-6
    os.remove(pred / "004.ply")
    proc = subprocess.run([sys.executable, "-m", "neuma_amd.particle_evaluation", "-p", str(pred), "-g", str(gt), "-k", "2",
                           "-n", "3"], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode != 0 and "004.ply" in proc.stderr
