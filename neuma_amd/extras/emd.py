"""The earth mover's distance of neuma_amd/particle_metrics.py (nm_emd, include/neuma_hip.h) stated in numpy: the twin of the
kernel (same assignment, prices and round count, bit for bit), the CPU path, and the yardstick of the tests.

EMD between two clouds a, b of n points each is a linear assignment problem.  Stated so that two implementations agree exactly:

  cost      c(i,j) = (dx*dx + dy*dy) + dz*dz in fp64 from the fp32 coordinates, in that order, no fma; power 1 takes its fp64 sqrt.
  scale     Cmax = the same expression on the extent of the joint bounding box of a and b; frexp(Cmax) = (m, ex), k = 24 - ex,
            C(i,j) = llrint(ldexp(c(i,j), k)): an int64 <= 2^24, scaled by an exact power of two.  The quantum 2^-k <= Cmax 2^-23
            is the rounding level of the fp32 inputs.  Cmax == 0 (all points identical): identity assignment, EMD 0, no rounds.
  solver    forward auction in Jacobi form with eps-scaling on Cs = C (n + 1), all int64: prices start at 0,
            eps0 = max(1, max(Cs) // 2), eps <- max(1, eps // 4) after each phase, the last phase has eps = 1; a phase starts with
            nobody assigned and keeps the prices.  In a round EVERY unassigned person i bids from the same price snapshot:
            v_j = -Cs(i,j) - price_j, j* the lowest j of maximal v, w1 = v_j*, w2 = max over j != j* (w2 = w1 for n = 1),
            bid = price_j* + (w1 - w2) + eps.  Per object the highest bid wins, the lowest person among equal bids; the winner takes
            the object, its previous owner becomes unassigned, the price becomes the bid.  A phase ends when nobody is unassigned.
  value     emd = mean_i c(i, sigma(i)) from the unquantised fp64 costs.

Guarantee (derived): at eps = 1 the result satisfies 1-complementary slackness on Cs, so sum Cs(i,sigma(i)) <= opt(Cs) + n, i.e.
sum C(i,sigma(i)) <= opt(C) + n/(n+1); both sides are integers, so the assignment is an exact optimum of the quantised problem.
Therefore the reported value exceeds the true fp64 optimum by at most 2^-k <= Cmax * 2^-23.

O(n^2) memory: for n up to a few thousand."""
import math

import numpy as np

BITS = 24
N_MAX = 8192
# default round limit = MAX_ROUNDS_PER_POINT * n: the largest rounds / n of the twin over tests/emd_cases.py (both powers) is
# 26672 / 256 = 104.19 (256 collinear points, power 1: on a line every monotone matching is optimal, so the bidders are nearly
# indifferent), times a 16x margin = 1667 (tests/test_emd_cpu.py holds the table to these numbers)
ROUNDS_PER_POINT_SEEN = 26672 / 256
ROUNDS_MARGIN = 16
MAX_ROUNDS_PER_POINT = 1667


def default_max_rounds(n: int) -> int:
    return MAX_ROUNDS_PER_POINT * int(n)


def _f64(a):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"expected an (n, 3) cloud, got {a.shape}")
    return a.astype(np.float32).astype(np.float64)


def _expr(d, power):
    c = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(c) if power == 1 else c


def _check(a, b, power):
    if power not in (1, 2):
        raise ValueError(f"power must be 1 or 2, got {power}")
    a, b = _f64(a), _f64(b)
    if a.shape != b.shape:
        raise ValueError(f"EMD needs clouds of equal size, got {a.shape[0]} and {b.shape[0]} points: subsample the larger one "
                         f"(particle_metrics.subsample_indices)")
    if not 1 <= a.shape[0] <= N_MAX:
        raise ValueError(f"n must be in [1, {N_MAX}], got {a.shape[0]}")
    return a, b


def costs(a, b, power):
    """c (n, n) fp64, unquantised"""
    a, b = _check(a, b, power)
    return _expr(a[:, None, :] - b[None, :, :], power)


def cost_scale(a, b, power):
    """(Cmax, k): the cost of the joint bounding box's extent and the power-of-two exponent of the quantisation"""
    a, b = _check(a, b, power)
    cmax = float(_expr(np.maximum(a.max(0), b.max(0)) - np.minimum(a.min(0), b.min(0)), power))
    return cmax, BITS - int(math.frexp(cmax)[1])


def quantised_costs(a, b, power):
    """(C int64 (n, n) <= 2^24, k) with C = llrint(ldexp(c, k))"""
    _, k = cost_scale(a, b, power)
    return np.rint(np.ldexp(costs(a, b, power), k)).astype(np.int64), k


def auction(C, max_rounds=None):
    """(idx (n) int64: person -> object, prices (n) int64 on Cs = C (n + 1), rounds) of the auction stated above.  Raises
    RuntimeError past max_rounds."""
    C = np.asarray(C, np.int64)
    n = C.shape[0]
    cs = C * (n + 1)
    price = np.zeros(n, np.int64)
    eps = max(1, int(cs.max()) // 2)
    rounds = 0
    lowest = np.iinfo(np.int64).min
    while True:
        owner = np.full(n, -1, np.int64)        # object -> person
        obj = np.full(n, -1, np.int64)          # person -> object
        while True:
            un = np.flatnonzero(obj < 0)
            if un.size == 0:
                break
            if max_rounds is not None and rounds >= max_rounds:
                raise RuntimeError(f"auction: round limit {max_rounds} reached")
            rows = np.arange(un.size)
            v = -cs[un] - price[None, :]
            j = np.argmax(v, 1)                 # the lowest j of maximal v
            w1 = v[rows, j]
            v[rows, j] = lowest
            w2 = v.max(1) if n > 1 else w1
            bid = price[j] + (w1 - w2) + eps
            order = np.lexsort((un, -bid, j))   # per object: highest bid first, lowest person among equal bids
            jj = j[order]
            first = np.r_[True, jj[1:] != jj[:-1]]
            wj, wp, wb = jj[first], un[order][first], bid[order][first]
            old = owner[wj]
            obj[old[old >= 0]] = -1
            owner[wj], obj[wp], price[wj] = wp, wj, wb
            rounds += 1
        if eps == 1:
            return obj, price, rounds
        eps = max(1, eps // 4)


def solve(a, b, power=1, max_rounds=None):
    """One item as nm_emd computes it: dict(emd, idx, prices, rounds, k, cmax).  A non-finite coordinate gives emd NaN, idx -1,
    rounds 0; identical points (Cmax == 0) the identity, emd 0, rounds 0."""
    a, b = _check(a, b, power)
    n = a.shape[0]
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return dict(emd=math.nan, idx=np.full(n, -1, np.int64), prices=np.zeros(n, np.int64), rounds=0, k=0, cmax=math.nan)
    cmax, k = cost_scale(a, b, power)
    if cmax == 0.0:
        return dict(emd=0.0, idx=np.arange(n, dtype=np.int64), prices=np.zeros(n, np.int64), rounds=0, k=k, cmax=0.0)
    c = costs(a, b, power)
    C = np.rint(np.ldexp(c, k)).astype(np.int64)
    idx, prices, rounds = auction(C, default_max_rounds(n) if max_rounds is None else max_rounds)
    return dict(emd=math.fsum(c[np.arange(n), idx]) / n, idx=idx, prices=prices, rounds=rounds, k=k, cmax=cmax)


def earth_movers_distance(a, b, power=1, give_id=False):
    """EMD of (n, 3) or batched (B, n, 3) CPU tensors / arrays: mean_i |a_i - b_sigma(i)|^power as a float (an fp64 array of B for
    a batch), with give_id also the assignment(s).  The value exceeds the true fp64 optimum by at most Cmax * 2^-23."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    if a.ndim == 3:
        if b.ndim != 3 or a.shape[0] != b.shape[0]:
            raise ValueError(f"batch sizes differ: {a.shape} and {b.shape}")
        res = [solve(x, y, power) for x, y in zip(a, b)]
        emd, idx = np.array([r["emd"] for r in res]), np.stack([r["idx"] for r in res])
        return (emd, idx) if give_id else emd
    r = solve(a, b, power)
    return (r["emd"], r["idx"]) if give_id else r["emd"]


def slackness_violation(C, idx, prices):
    """max over i of  max_j(-Cs(i,j) - p_j) - (-Cs(i,sigma(i)) - p_sigma(i)):  <= 1 certifies the assignment (1-complementary
    slackness on Cs = C (n + 1)), hence exact optimality on C."""
    C = np.asarray(C, np.int64)
    n = C.shape[0]
    v = -C * (n + 1) - np.asarray(prices, np.int64)[None, :]
    return int((v.max(1) - v[np.arange(n), np.asarray(idx)]).max())
