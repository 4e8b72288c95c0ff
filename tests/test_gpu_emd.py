"""GPU: the exact assignment auction of csrc/nm_emd.hip (nm_emd) through neuma_amd.particle_metrics - bitwise against its numpy
twin (neuma_amd/extras/emd.py) and against scipy's exact solver on every case of tests/emd_cases.py, certified from its own
prices at n = 8192, batched, with non-finite items, repeated, at the round limit, on bad arguments, through autograd - and
`python -m neuma_amd.particle_evaluation --emd` end to end."""
import contextlib
import functools
import io
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import emd_cases as K
from gpu_util import dev, measured, rel_max

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CASE_POWER = [(name, p) for name in K.CASES for p in K.POWERS]


def _pm():
    from neuma_amd import particle_metrics
    return particle_metrics


def _g(a):
    return torch.from_numpy(np.array(a)).to(dev())        # (a copy: the cases are read-only arrays)


@functools.lru_cache(maxsize=None)
def native(name, power):
    """(emd, idx, rounds, prices) of one case alone, as numpy / python values: one nm_emd call per case and power, shared"""
    a, b = K.case(name)
    emd, idx, rounds, prices = _pm().emd_native(_g(a)[None], _g(b)[None], power=power, give_prices=True)
    return float(emd[0]), idx[0].cpu().numpy(), int(rounds[0]), prices[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def scipy_optimum(name, power):
    C = K.twin(name, power)["C"]
    r, c = linear_sum_assignment(C)
    return int(C[r, c].sum())


@pytest.mark.parametrize("name,power", CASE_POWER)
def test_twin_parity_bitwise(name, power):
    t = K.twin(name, power)
    emd, idx, rounds, prices = native(name, power)
    print(f"{name} p={power}: rounds {rounds} (twin {t['rounds']}), emd {emd!r} (twin {t['emd']!r})")
    assert measured(int((idx != t["idx"]).sum()), "idx entries that differ from the twin") <= 0
    assert measured(int((prices != t["prices"]).sum()), "prices that differ from the twin") <= 0
    assert measured(abs(rounds - t["rounds"]), "rounds - twin rounds") <= 0
    # the fp64 gather value: the exactly rounded sum of the unquantised costs of the assignment, over n
    assert measured(abs(emd - t["emd"]) / max(abs(t["emd"]), 1e-300) if t["emd"] != 0.0 else abs(emd), "emd vs fp64 gather") <= 1e-15


@pytest.mark.parametrize("name,power", CASE_POWER)
def test_assignment_is_scipys_optimum(name, power):
    n, C = K.CASES[name][1], K.twin(name, power)["C"]
    _, idx, _, _ = native(name, power)
    assert sorted(idx.tolist()) == list(range(n)), "idx is not a permutation"
    mine = int(C[np.arange(n), idx].sum())
    assert measured(abs(mine - scipy_optimum(name, power)), "sum C - scipy optimum") <= 0         # integer equality


def _device_certificate(a, b, power, idx, prices):
    """max_i [ max_j(-Cs(i,j) - p_j) - (-Cs(i,idx(i)) - p_idx(i)) ] in torch int64 on the device, C by the formula of
    extras.emd.quantised_costs (every operation a separate fp64 kernel, so nothing is contracted); <= 1 certifies optimality"""
    from neuma_amd.extras import emd as E
    n = a.shape[0]
    _, k = E.cost_scale(a, b, power)
    ad, bd = _g(a).double(), _g(b).double()
    worst = 0
    for r0 in range(0, n, 1024):
        d = ad[r0:r0 + 1024, None, :] - bd[None, :, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        c = (dx * dx + dy * dy) + dz * dz
        if power == 1:
            c = torch.sqrt(c)
        cs = torch.round(c * 2.0 ** k).long() * (n + 1)             # 2^k is exact: ldexp
        v = -cs - prices[None, :]
        mine = torch.gather(v, 1, idx[r0:r0 + 1024, None])[:, 0]
        worst = max(worst, int((v.max(1).values - mine).max()))
    return worst


@pytest.mark.parametrize("kind,power", [("uniform", 1), ("clusters", 2)])
def test_largest_size_certified_from_its_prices(kind, power):
    """n = 8192 is beyond scipy and the twin: the assignment is certified from the returned prices alone.  Each cloud pair runs
    with one exponent so that both kernels meet the largest size (uniform, power 1: 36 k rounds; clusters, power 2: 74 k rounds;
    the clusters' power-1 price war is 207 k rounds, 9 s on one compute unit, and adds no code path)."""
    n = 8192
    a, b = K.uniform(n) if kind == "uniform" else K.clusters(n)
    emd, idx, rounds, prices = _pm().emd_native(_g(a)[None], _g(b)[None], power=power, give_prices=True)
    print(f"{kind} n={n} p={power}: rounds {int(rounds[0])} ({int(rounds[0]) / n:.2f} n), emd {float(emd[0])!r}, "
          f"max price 2^{math.log2(max(1, int(prices.max()))):.1f}")
    assert sorted(idx[0].tolist()) == list(range(n)), "idx is not a permutation"
    assert int(rounds[0]) > 0 and math.isfinite(float(emd[0]))
    assert measured(_device_certificate(a, b, power, idx[0], prices[0]), "slackness violation") <= 1


def test_certificate_agrees_with_the_twins_formula():
    """the device certificate of the n = 8192 test, on a case small enough for the twin: same C, same verdict"""
    from neuma_amd.extras import emd as E
    for power in K.POWERS:
        a, b = K.case("uniform65")
        t = K.twin("uniform65", power)
        got = _device_certificate(a, b, power, _g(t["idx"]), _g(t["prices"]))
        assert got == E.slackness_violation(t["C"], t["idx"], t["prices"])
        wrong = np.roll(t["idx"], 1)
        assert _device_certificate(a, b, power, _g(wrong), _g(t["prices"])) > 1


def test_batch_equals_each_item_alone_and_nan_item():
    names = ["uniform256", "permuted_jitter256", "collinear256"]
    a = np.stack([K.case(nm)[0] for nm in names])
    b = np.stack([K.case(nm)[1] for nm in names])
    emd, idx, rounds, prices = _pm().emd_native(_g(a), _g(b), power=1, give_prices=True)
    for i, nm in enumerate(names):
        e1, i1, r1, p1 = native(nm, 1)
        assert float(emd[i]) == e1 and int(rounds[i]) == r1
        assert np.array_equal(idx[i].cpu().numpy(), i1) and np.array_equal(prices[i].cpu().numpy(), p1)
    bad = a.copy()
    bad[1, 17, 2] = np.nan
    emd2, idx2, rounds2 = _pm().emd_native(_g(bad), _g(b), power=1)
    assert math.isnan(float(emd2[1])) and bool((idx2[1] == -1).all()) and int(rounds2[1]) == 0
    for i in (0, 2):
        assert float(emd2[i]) == float(emd[i]) and int(rounds2[i]) == int(rounds[i]) and torch.equal(idx2[i], idx[i])
    bad[1, 17, 2] = np.inf
    emd3, _, _ = _pm().emd_native(_g(b), _g(bad), power=2)
    assert math.isnan(float(emd3[1])) and math.isfinite(float(emd3[0])) and math.isfinite(float(emd3[2]))
    v = _pm().earth_movers_distance(_g(b), _g(bad), power=2)
    assert math.isnan(float(v[1])) and math.isfinite(float(v[0]))


def test_two_calls_are_bitwise_equal():
    a, b = K.case("ties1024")
    x = _pm().emd_native(_g(a)[None], _g(b)[None], power=2, give_prices=True)
    first = native("ties1024", 2)
    assert float(x[0][0]).hex() == first[0].hex() and int(x[2][0]) == first[2]
    assert np.array_equal(x[1][0].cpu().numpy(), first[1]) and np.array_equal(x[3][0].cpu().numpy(), first[3])


def test_round_limit_is_a_status_not_a_fault():
    from neuma_amd import NeumaHipError
    a, b = K.case("clusters1024")
    u = K.case("uniform64")
    same = np.tile(a[:1], (len(a), 1))           # item 0: identical points need no round at all
    with pytest.raises(NeumaHipError, match=r"item 1 reached the round limit \(max_rounds = 4\)"):
        _pm().emd_native(_g(np.stack([same, a])), _g(np.stack([same, b])), power=1, max_rounds=4)
    emd, idx, rounds = _pm().emd_native(_g(u[0])[None], _g(u[1])[None], power=1)                 # the process carries on
    first = native("uniform64", 1)
    assert float(emd[0]) == first[0] and int(rounds[0]) == first[2] and np.array_equal(idx[0].cpu().numpy(), first[1])


def test_arguments_are_rejected_with_their_messages():
    from neuma_amd import NeumaHipError, _lib
    pm = _pm()
    z = torch.zeros(1, 8193, 3, device=dev())
    with pytest.raises(ValueError, match="empty point cloud"):
        pm.emd_native(z[:, :0], z[:, :0])
    with pytest.raises(NeumaHipError, match=r"n must be in \[1, 8192\], got 8193"):
        pm.emd_native(z, z)
    with pytest.raises(ValueError, match="at most 8192"):
        pm.earth_movers_distance(z, z)
    with pytest.raises(NeumaHipError, match="power must be 1 or 2, got 3"):
        pm.emd_native(z[:, :8], z[:, :8], power=3)
    with pytest.raises(ValueError, match="power must be 1 or 2"):
        pm.earth_movers_distance(z[:, :8], z[:, :8], power=3)
    with pytest.raises(ValueError, match="subsample"):
        pm.emd_native(z[:, :8], z[:, :9])
    with pytest.raises(ValueError, match="subsample"):
        pm.earth_movers_distance(z[:, :8], z[:, :9])
    with pytest.raises(NeumaHipError, match="GPU"):
        pm.emd_native(z[:, :8].cpu(), z[:, :8].cpu())
    lib = _lib.lib()
    assert lib.nm_emd_workspace(1, 0) == 0 and lib.nm_emd_workspace(1, 8193) == 0 and lib.nm_emd_workspace(3, 8192) >= 12
    out = torch.zeros(64, dtype=torch.int64, device=dev())
    p = z[:, :8].contiguous()
    args = (p.data_ptr(), p.data_ptr(), out.data_ptr(), out[8:].data_ptr(), None, out[32:].data_ptr(), out[40:].data_ptr())
    assert lib.nm_emd(1, 0, 1, 100, *args, 256, None) == -1 and b"n must be in [1, 8192]" in lib.nm_last_error()
    assert lib.nm_emd(1, 8, 1, 100, *args, 0, None) == -1 and b"workspace too small" in lib.nm_last_error()
    assert lib.nm_emd(1, 8, 1, 0, *args, 256, None) == -1 and b"max_rounds" in lib.nm_last_error()


@pytest.mark.parametrize("power", K.POWERS)
def test_gradient_flows_through_the_gather(power):
    a0, b0 = K.case("uniform65")
    a0, b0 = np.stack([a0, b0]).astype(np.float64), np.stack([b0, a0[::-1]]).astype(np.float64)
    w = torch.tensor([1.0, -0.5], dtype=torch.float64, device=dev())
    a, b = _g(a0).requires_grad_(), _g(b0).requires_grad_()
    val, idx = _pm().earth_movers_distance(a, b, power=power, give_id=True)
    assert val.dtype == torch.float64 and val.shape == (2,) and not idx.requires_grad
    (val * w).sum().backward()
    # torch fp64 on the CPU with the same indices: 2 (x - y_s) / n for power 2, the unit vectors over n for power 1, and
    # their scatter on the other cloud
    n = a0.shape[1]
    x, y, s = torch.from_numpy(a0), torch.from_numpy(b0), idx.cpu()
    diff = x - torch.gather(y, 1, s[..., None].expand(-1, -1, 3))
    gx = (2.0 * diff if power == 2 else diff / diff.norm(dim=2, keepdim=True)) * (w.cpu().view(2, 1, 1) / n)
    gy = torch.zeros_like(y).scatter_add_(1, s[..., None].expand(-1, -1, 3), -gx)
    ref = (diff.pow(2).sum(2) if power == 2 else diff.norm(dim=2)).mean(1)
    assert rel_max(val, ref) < 1e-14
    assert rel_max(a.grad, gx) < 1e-13
    assert rel_max(b.grad, gy) < 1e-13
    af, bf = _g(a0.astype(np.float32)).requires_grad_(), _g(b0.astype(np.float32)).requires_grad_()
    vf = _pm().earth_movers_distance(af, bf, power=power)
    vf.sum().backward()
    assert vf.dtype == torch.float32 and bool(torch.isfinite(af.grad).all()) and bool(torch.isfinite(bf.grad).all())
    # coincident points (an exact permutation): value exactly 0 and a finite (zero) gradient for both powers
    p, q = K.case("exact_permutation512")
    pt, qt = _g(p)[None].requires_grad_(), _g(q)[None].requires_grad_()
    v0 = _pm().earth_movers_distance(pt, qt, power=power)
    v0.sum().backward()
    assert float(v0.detach()[0]) == 0.0 and not bool(pt.grad.any()) and not bool(qt.grad.any())


def test_entry_point_end_to_end(tmp_path):
    from neuma_amd import particle_evaluation as pe
    from neuma_amd.io import load_particles_ply, save_particles_ply
    r = np.random.Generator(np.random.PCG64(31))
    pred, gt = tmp_path / "states_run", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    sizes = {0: (300, 250), 1: (300, 250), 2: (100, 250)}
    for i, (n, m) in sizes.items():
        save_particles_ply(pred / f"{i:03d}.ply", r.uniform(0, 1, (n, 3)).astype(np.float32))
        save_particles_ply(gt / f"{i:03d}.ply", (r.uniform(0, 1, (m, 3)) * 1.1).astype(np.float32))
    cmd = [sys.executable, "-m", "neuma_amd.particle_evaluation", "-p", str(pred), "-g", str(gt), "-n", "2"]
    env = dict(os.environ)

    # the untouched Chamfer path, run here: the driver's own helpers, none of which the EMD option changed
    frames = pe.frame_indices(0, 1, 2)
    paths = [pe.frame_paths(str(pred), str(gt), i) for i in frames]
    preds, gts = [load_particles_ply(p) for p, _ in paths], [load_particles_ply(g) for _, g in paths]
    c12, c21 = [0.0] * 3, [0.0] * 3
    for grp in pe.group_frames([(len(p), len(g)) for p, g in zip(preds, gts)]):
        va, vb = pe._score([preds[k] for k in grp], [gts[k] for k in grp], dev())
        for k, x, y in zip(grp, va, vb):
            c12[k], c21[k] = x, y
    cd = [x + y for x, y in zip(c12, c21)]
    want = tmp_path / "want_chamfer.txt"
    pe.write_metrics(str(want), frames, cd, c12, c21)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        print(f"current pred_dir: {pred}, skip: 1, from 0 to 2")
        for i, p, g, v, x, y in zip(frames, preds, gts, cd, c12, c21):
            print(f"pr: {i:03d}.ply [{len(p)}] | gt: {i:03d}.ply [{len(g)}] | CD: {v:.6e} | pred->gt: {x:.6e} | gt->pred: {y:.6e}")
        print(f"mean CD: {sum(cd) / len(cd):.6e}")

    plain = subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert plain.stdout == out.getvalue()
    assert (tmp_path / "states_run_chamfer.txt").read_bytes() == want.read_bytes()
    assert not (tmp_path / "states_run_emd.txt").exists()

    full = subprocess.run(cmd + ["--emd", "--emd_points", "128"], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert full.returncode == 0, full.stdout[-2000:] + full.stderr[-2000:]
    assert (tmp_path / "states_run_chamfer.txt").read_bytes() == want.read_bytes()
    lines = full.stdout.splitlines()
    assert [ln.split(" | EMD: ")[0] for ln in lines[:5]] == plain.stdout.splitlines()
    assert all(" | EMD: " in ln for ln in lines[1:4]) and " | EMD: " not in lines[0] + lines[4]
    assert lines[5].startswith("mean EMD: ") and "n: 100/128" in lines[5] and "power: 1" in lines[5] and "seed: 0" in lines[5]
    rows = [ln.split() for ln in (tmp_path / "states_run_emd.txt").read_text().splitlines()]
    assert rows[0] == ["frame", "EMD", "n", "rounds"] and [x[0] for x in rows[1:]] == ["000", "001", "002", "mean"]
    pm, ref, bounds = _pm(), [], []
    for k, (p, g) in enumerate(zip(preds, gts)):
        n = min(len(p), len(g), 128)
        sp, sg = pm.subsample_indices(len(p), n, 0), pm.subsample_indices(len(g), n, 0)
        emd, _, rounds = pm.emd_native(_g(np.asarray(p, np.float32)[sp])[None], _g(np.asarray(g, np.float32)[sg])[None], power=1)
        ref.append(float(emd[0]))
        both = np.concatenate([np.asarray(p, np.float32)[sp], np.asarray(g, np.float32)[sg]]).astype(np.float64)
        e = both.max(0) - both.min(0)
        bounds.append(float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) * 2.0 ** -23)          # Cmax 2^-23, power 1
        assert rows[1 + k][1] == f"{ref[-1]:.8e}" and int(rows[1 + k][2]) == n and int(rows[1 + k][3]) == int(rounds[0])
        assert f" | EMD: {ref[-1]:.6e}" in lines[1 + k]
    assert rows[4] == ["mean", f"{sum(ref) / 3:.8e}"]
    assert f"at most {max(bounds):.3e} above" in lines[5]
