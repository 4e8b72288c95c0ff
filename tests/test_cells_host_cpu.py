"""CPU: the HOST half of nm_cells_fit / nm_cell (csrc/nm_cells.h, both __host__ __device__) over seeded boxes and budgets for
D = 2 and D = 3.  tests/cells_host/cells_host_main.hip is built into tmp_path and run as a program; it makes no HIP call.

What this does NOT cover: the device's pow / sqrt, which may round the cell edge differently (a cell count one off, still within
the budget: the shrink loop is the same code).  The device path is held by the GPU suites of the files that bin
(tests/test_gpu_cells.py and its neighbours), whose results do not depend on the cell counts.

The bounds are derived, not measured: with h the cubic cell edge over the active axes A, prod_A (e_k / h) = cmax, and
floor(t) >= t / 2 for t >= 2, so prod n_k >= cmax / 2^|A| >= cmax / 2^D whenever every active axis is two edges long; the
shrink loop only runs above the budget and its last step leaves more than half of it."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cells_host" / "cells_host_main.hip"
BUDGETS = (1, 2, 3, 7, 64, 1 << 20, 1 << 26)
RANDOM_PER_BUDGET = 120
PROBES = 25          # per axis: 24 sorted coordinates from -Inf to +Inf, then NaN
DMAX = 1.7976931348623157e308


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


def boxes(D, seed):
    """(lo, hi, cmax) rows: extents 1e-30 .. 1e30, aspect ratios up to 1e12, origins at 0, near and far from the box's own
    size, and with every budget the special boxes: zero-extent axes, lo > hi, an extent beyond the fp64 range."""
    rng = np.random.default_rng(seed)
    lo, hi, cm = [], [], []
    for cmax in BUDGETS:
        for i in range(RANDOM_PER_BUDGET):
            long_side = 10.0 ** rng.uniform(-18, 30)
            e = long_side * 10.0 ** -rng.uniform(0, 12, D)
            e[rng.integers(D)] = long_side
            if i % 10 == 0:
                e[:] = 10.0 ** rng.uniform(-30, 30)                   # a cube
            if i % 10 == 1:
                e = e / e.max() * 10.0 ** rng.choice([-30.0, 30.0])   # the ends of the range
            o = e * rng.uniform(-3, 3, D) * rng.choice([0.0, 1.0, 1e3])
            lo.append(o); hi.append(o + e); cm.append(cmax)
        one = np.ones(D)
        for k in range(D):
            z = one.copy(); z[k] = 0.0
            lo.append(-z); hi.append(z); cm.append(cmax)                             # one axis of extent zero
            lo.append(one * 0.25); hi.append(one * 0.25 + (1 - z) * 3.0); cm.append(cmax)   # all axes but one
            a = one.copy(); a[k] = -1.0
            lo.append(one.copy()); hi.append(2 * a); cm.append(cmax)                 # lo > hi on one axis
            lo.append(np.where(a < 0, np.inf, 0.0)); hi.append(np.where(a < 0, -np.inf, 5.0)); cm.append(cmax)   # nothing finite
            lo.append(np.where(a < 0, -1.5e308, -1.0)); hi.append(np.where(a < 0, 1.5e308, 1.0)); cm.append(cmax)  # overflow
        lo.append(np.zeros(D)); hi.append(np.zeros(D)); cm.append(cmax)              # a point
        lo.append(np.full(D, np.inf)); hi.append(np.full(D, -np.inf)); cm.append(cmax)
        lo.append(np.full(D, -1.5e308)); hi.append(np.full(D, 1.5e308)); cm.append(cmax)
    return np.array(lo), np.array(hi), np.array(cm, dtype=np.float64)


def probes(lo, hi, seed):
    """(n, D, PROBES): per axis 24 ascending coordinates (-Inf, below the box, lo, inside, hi, above, +Inf), then NaN."""
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        e = np.where(lo <= hi, hi - lo, 0.0)
        a = np.where(lo <= hi, lo, 0.0)
        b = np.where(lo <= hi, hi, 0.0)
        far = 1e3 * (np.abs(a) + np.abs(b) + 1.0)
        t = rng.uniform(0, 1, lo.shape + (14,))
        inside = a[..., None] * (1 - t) + b[..., None] * t
        inside = np.where(np.isfinite(inside), np.clip(inside, a[..., None], b[..., None]), a[..., None])
        cols = [np.full(lo.shape, -np.inf), a - far, a - 0.5 * e, np.nextafter(a, -np.inf), a, b, np.nextafter(b, np.inf),
                b + 0.5 * e, b + far, np.full(lo.shape, np.inf)]
        x = np.concatenate([np.stack(cols, -1), inside], -1)
    x = np.sort(np.where(np.isnan(x), a[..., None], x), -1)
    return np.concatenate([x, np.full(lo.shape + (1,), np.nan)], -1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("cells_host") / "cells_host_main"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", str(SRC), "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module", params=[2, 3])
def fitted(request, exe):
    D = request.param
    lo, hi, cmax = boxes(D, 100 + D)
    x = probes(lo, hi, 200 + D)
    n = lo.shape[0]
    d = exe.parent
    rec = np.concatenate([lo, hi, cmax[:, None], x.reshape(n, D * PROBES)], 1)
    with open(d / f"in{D}.bin", "wb") as fh:
        fh.write(np.array([D, n, PROBES], dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(rec, dtype=np.float64).tobytes())
    subprocess.run([str(exe), str(d / f"in{D}.bin"), str(d / f"out{D}.bin")], check=True, timeout=60)
    raw = np.fromfile(d / f"out{D}.bin", dtype=np.float64)
    assert raw.size == n * (6 * D + D * PROBES)
    raw = raw.reshape(n, -1)
    f = {name: raw[:, i * D:(i + 1) * D] for i, name in enumerate(("lo", "hi", "e", "o", "inv_h", "n"))}
    f["cell"] = raw[:, 6 * D:].reshape(n, D, PROBES)
    f.update(D=D, lo_in=lo, hi_in=hi, cmax=cmax, x=x)
    return f


def test_boxes_cover_what_they_should():
    for D in (2, 3):
        lo, hi, cmax = boxes(D, 100 + D)
        with np.errstate(all="ignore"):
            e = hi - lo
        ok = np.isfinite(e) & (e > 0)
        assert set(cmax.astype(np.int64)) == set(BUDGETS)
        assert e[ok].min() <= 1e-29 and e[ok].max() >= 1e29
        full = ok.all(1)
        assert (e[full].max(1) / e[full].min(1)).max() >= 1e11
        assert (e == 0).any() and (lo > hi).any() and np.isinf(e).any()


def test_counts_are_within_the_budget_and_degenerate_axes_get_one_cell(fitted):
    f = fitted
    n, e, cmax = f["n"], f["e"], f["cmax"]
    assert (n == np.floor(n)).all() and (n >= 1).all()
    assert (np.prod(n, 1) <= cmax).all()
    empty = ~(f["lo_in"] <= f["hi_in"])
    assert (f["lo"][empty] == 0).all() and (f["hi"][empty] == 0).all() and (e[empty] == 0).all()
    assert (f["lo"][~empty] == f["lo_in"][~empty]).all() and (f["hi"][~empty] == f["hi_in"][~empty]).all()
    assert (f["o"] == f["lo"]).all()
    with np.errstate(all="ignore"):
        assert (e == f["hi"] - f["lo"]).all()
        real = (e > 0) & (e <= DMAX)
        assert (n[~real] == 1).all() and (f["inv_h"][~real] == 0).all()
        assert (f["inv_h"][real] == (n / e)[real]).all()


def _ideal_edge(e, cmax):
    """the rule in logarithms: the cubic edge over the active axes, an axis shorter than it dropped, repeated"""
    active = (e > 0) & (e <= DMAX)
    h = np.inf
    for _ in range(e.size):
        if not active.any():
            break
        h = np.exp((np.log(e[active]).sum() - np.log(cmax)) / active.sum())
        short = active & (e < h)
        if not short.any():
            break
        active &= ~short
    return h, active


def test_the_budget_is_used(fitted):
    f = fitted
    D, used, applies = f["D"], [], 0
    for i in range(f["n"].shape[0]):
        h, active = _ideal_edge(f["e"][i], f["cmax"][i])
        if active.any() and (f["e"][i][active] >= 2.0 * (1 + 1e-9) * h).all():      # (clear of the edge of the hypothesis)
            applies += 1
            used.append(np.prod(f["n"][i]) / f["cmax"][i])
            assert np.prod(f["n"][i]) >= f["cmax"][i] / 2 ** D, (i, f["e"][i], f["cmax"][i], f["n"][i])
    print(f"D={D}: bound applies to {applies} of {f['n'].shape[0]} boxes, least use {min(used):.3f} of the budget")
    assert applies >= 100


def test_cell_map_is_monotone_and_clamped(fitted):
    f = fitted
    x, cell, n = f["x"], f["cell"], f["n"]
    assert (cell == np.floor(cell)).all() and (cell >= 0).all() and (cell <= n[..., None] - 1).all()
    srt, c = x[..., :-1], cell[..., :-1]
    assert (srt[..., 1:] >= srt[..., :-1]).all() and (c[..., 1:] >= c[..., :-1]).all()
    assert (c[srt <= f["lo"][..., None]] == 0).all()                                   # lo itself, below it, -Inf
    top = np.broadcast_to(n[..., None] - 1, c.shape)
    assert (c[srt >= f["hi"][..., None]] == top[srt >= f["hi"][..., None]]).all()      # hi itself, above it, +Inf
    assert (srt[..., 0] == -np.inf).all() and (srt[..., -1] == np.inf).all()
    assert np.isnan(x[..., -1]).all() and (cell[..., -1] == 0).all()
