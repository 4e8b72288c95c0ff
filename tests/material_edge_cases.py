"""Inputs and fp64 references for the constitutive kernels (nm_material.hip) at every edge of their work split.
Importable without a GPU: tests/test_material_edges_cpu.py checks the case list and the references themselves,
tests/test_gpu_material_edges.py holds the kernels to them.

The work split (nm_wave_quota, NM_BWD_GRID = 256): a wave owns q = ceil(n / 1024) rounded up to 16 consecutive particles, a
workgroup is four waves, a wave runs rounds of 64 particles = 1..4 tiles of 16.  Every per-particle quantity (forward value,
dL/dF) depends on its own row alone, and the weight gradient is a sum over rows: all references are therefore taken from ONE
set of n_max rows, a case of n particles uses the first n of them, and the fp64 passes are run once per stretch of rows
between two case counts (`PrefixRef`) - no row goes through the oracle twice."""
import bisect
from pathlib import Path

import numpy as np
import torch

from oracle import material as om

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = ("jelly", "plasticine", "sand")
KINDS = ("e", "p")
ALPHA = 1e-3

NM_BWD_GRID = 256          # tests/test_gpu_material_edges.py asserts this against nm_material_bwd_workspace
NM_WACC = 6144             # floats of one workgroup's partial weight gradient
NM_PRO_WGS = 32
CLAMP = 1e-6               # |s_j^2 - s_i^2| below which the reference's SVD adjoint clamps its denominators


def wave_quota(n):
    """(grid, q) of nm_wave_quota"""
    waves = NM_BWD_GRID * 4
    q = (n + waves - 1) // waves
    q = ((q + 15) // 16) * 16
    q = max(q, 16)
    grid = max((n + 4 * q - 1) // (4 * q), 1)
    return grid, q


def geometry(n):
    grid, q = wave_quota(n)
    full, rest = divmod(q, 64)
    rounds = (["4"] if full else []) + ([str(rest // 16)] if rest else [])      # a full wave's rounds: q <= 96 here
    assert full <= 1
    last_wg = n - (grid - 1) * 4 * q
    return dict(grid=grid, q=q, tiles_per_round=" + ".join(rounds), last_wave=n - ((n - 1) // q) * q,
                last_tile=(n - 1) % 16 + 1, split=grid + NM_PRO_WGS <= NM_BWD_GRID, last_wg_waves_1_to_3_empty=last_wg <= q)


# n: (grid, q, tiles per round, last wave holds, prologue split) - the table of the work split's edges, literal
TABLE = {
    1: (1, 16, "1", 1, True),
    15: (1, 16, "1", 15, True), 16: (1, 16, "1", 16, True), 17: (1, 16, "1", 1, True),
    63: (1, 16, "1", 15, True), 64: (1, 16, "1", 16, True), 65: (2, 16, "1", 1, True),
    255: (4, 16, "1", 15, True), 256: (4, 16, "1", 16, True), 257: (5, 16, "1", 1, True),
    14_336: (224, 16, "1", 16, True), 14_337: (225, 16, "1", 1, False),
    16_383: (256, 16, "1", 15, False), 16_384: (256, 16, "1", 16, False),
    16_385: (129, 32, "2", 1, True),
    32_768: (256, 32, "2", 32, False), 32_769: (171, 48, "3", 33, True),
    49_153: (193, 64, "4", 1, True),
    65_536: (256, 64, "4", 64, False), 65_537: (205, 80, "4 + 1", 17, True),
    81_921: (214, 96, "4 + 2", 33, True),
}
# k_wgrad_reduce: wave sl sums partials sl, sl + 4, ... in a loop unrolled by 16 (`b + 12 < nparts`) plus a tail; these
# numbers of partials take every exit of both loops for each of the four slices
REDUCE_PARTS = (1, 2, 3, 4, 5, 12, 13, 14, 16, 17, 28, 29, 32, 33)
REDUCE_CASES = {64 * k: k for k in REDUCE_PARTS}
REDUCE_CASES.update({64 * k - 63: k for k in (2, 5, 13, 17, 29, 33)})      # ... with one particle in the last workgroup
CASES = tuple(sorted(set(TABLE) | set(REDUCE_CASES)))
N_MAX = max(CASES)
POLAR_CASES = (17, 16_383, 65_537)          # a partial tile, the unsplit prologue's count, two rounds
MISALIGNED_CASES = (17, 257, 16_385)


def coverage_gaps(cases=CASES):
    """classes of the work split that no case of `cases` reaches ([] = the list is complete)"""
    geo = {n: geometry(n) for n in cases}
    want = {}
    for fill in (1, 15, 16):
        want[f"last tile holds {fill}"] = any(g["last_tile"] == fill for g in geo.values())
    want["a workgroup whose waves 1 to 3 are empty"] = any(g["last_wg_waves_1_to_3_empty"] for g in geo.values())
    for t in ("1", "2", "3", "4", "4 + 1", "4 + 2"):
        want[f"tiles per round {t}"] = any(g["tiles_per_round"] == t for g in geo.values())
    for qa, qb in ((16, 32), (32, 48), (64, 80)):
        want[f"q {qa} -> {qb}, both sides"] = any(n in geo and n + 1 in geo and geo[n]["q"] == qa and geo[n + 1]["q"] == qb
                                                   for n in cases)
    want["grid 256"] = any(g["grid"] == NM_BWD_GRID for g in geo.values())
    want["split prologue"] = any(g["split"] for g in geo.values())
    want["unsplit prologue"] = any(not g["split"] for g in geo.values())
    for k in REDUCE_PARTS:
        want[f"{k} partials"] = any(g["grid"] == k and g["q"] == 16 for g in geo.values())
    return [k for k, ok in want.items() if not ok]


def boundary_rows(n):
    """the particles next to a boundary of the work split (tile, wave, round, workgroup, end), plus - for the reduce cases -
    the first particle of every workgroup, so that every partial carries exactly one known term"""
    grid, q = wave_quota(n)
    rows = {0, 15, 16, q - 1, q, 63, 64, 4 * q - 1, 4 * q, n - 17, n - 16, n - 2, n - 1}
    if n in REDUCE_CASES:
        rows |= {4 * q * b for b in range(grid)}
    return sorted(r for r in rows if 0 <= r < n)


# ---------------------------------------------------------------- inputs
def _rotations(n, gen):
    Q, R = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))
    Q = Q * torch.sign(torch.diagonal(R, dim1=1, dim2=2))[:, None, :]
    return Q * torch.sign(torch.linalg.det(Q))[:, None, None]


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def separated_F():
    """(N_MAX, 3, 3) fp64 holding fp32 values: F = U diag(s) V^T, random rotations, singular values >= 0.1 apart in
    [0.6, 1.5] - the clamp of the reference's SVD adjoint is inactive, fp64 autograd through torch.linalg.svd is the truth"""
    def make():
        gen = torch.Generator().manual_seed(20)
        u = torch.rand(N_MAX, 3, generator=gen, dtype=torch.float64)
        s2 = 0.6 + 0.15 * u[:, 0]
        s1 = s2 + 0.1 + 0.25 * u[:, 1]
        s0 = s1 + 0.1 + 0.25 * u[:, 2]
        F = _rotations(N_MAX, gen) @ torch.diag_embed(torch.stack([s0, s1, s2], 1)) @ _rotations(N_MAX, gen).transpose(1, 2)
        return F.float().double()
    return _once("F", make)


def dense_gout():
    return _once("go", lambda: torch.randn(N_MAX, 3, 3, generator=torch.Generator().manual_seed(21)).double())


def boundary_gout(n):
    """(n, 3, 3) fp64 holding fp32 values, non-zero on boundary_rows(n) only"""
    rows = boundary_rows(n)
    g = torch.zeros(n, 3, 3, dtype=torch.float64)
    g[rows] = torch.randn(len(rows), 3, 3, generator=torch.Generator().manual_seed(22 + n)).double()
    return g


DEGENERATE_PERIOD = 45      # odd, no divisor of 16: every kind of row visits every lane of a tile


def degenerate_F(n):
    """(n, 3, 3): F = I, diag(a, a, b), diag(a, b, b) and rotated copies of them, repeating with period 45"""
    def make():
        gen = torch.Generator().manual_seed(23)
        P = DEGENERATE_PERIOD
        ab = 0.8 + 0.5 * torch.rand(P, 2, generator=gen, dtype=torch.float64)
        F = torch.eye(3, dtype=torch.float64).repeat(P, 1, 1)
        F[1::5] = torch.diag_embed(torch.stack([ab[1::5, 0], ab[1::5, 0], ab[1::5, 1]], 1))
        F[2::5] = torch.diag_embed(torch.stack([ab[2::5, 0], ab[2::5, 1], ab[2::5, 1]], 1))
        Q = _rotations(P, gen)
        F[3::5] = Q[3::5] @ F[1::5] @ Q[3::5].transpose(1, 2)
        F[4::5] = Q[4::5] @ F[2::5] @ Q[4::5].transpose(1, 2)
        return F.float().double()
    return _once("Fdeg", make)[torch.arange(n) % DEGENERATE_PERIOD]


def degenerate_forward_ref(name, kind, n):
    def make():
        with torch.no_grad():
            return _apply(kind, degenerate_F(DEGENERATE_PERIOD), weights(name, kind, lora=False))
    return _once(("deg", name, kind), make)[torch.arange(n) % DEGENERATE_PERIOD]


def weights(name, kind, lora):
    """the three matrices the kernel is given, as fp64 copies of their fp32 values: a shipped checkpoint, optionally with the
    golden LoRA factors merged in (W + s B A rounded to fp32 once - the same numbers go to the GPU and to the oracle)"""
    def make():
        b = np.load(GOLDEN / "base_models.npz")
        W = [torch.tensor(b[f"{name}_{kind}_w{i}"]).double() for i in range(3)]
        if lora:
            g = np.load(GOLDEN / f"material_{name}.npz")
            W = [om.lora_effective_weight(w, torch.tensor(g[f"{kind}_A{i}"]).double(), torch.tensor(g[f"{kind}_B{i}"]).double(),
                                          float(g[f"{kind}_scaling"])) for i, w in enumerate(W)]
        return [w.float().double() for w in W]
    return _once(("W", name, kind, lora), make)


def _apply(kind, F, W):
    return om.elasticity(F, W) if kind == "e" else om.plasticity(F, W, ALPHA)


def per_rows_ref(kind, F, gout, W, dtype=torch.float64):
    """autograd of L = <net(F), gout> through the oracle, run in `dtype`: (out, dL/dF, [dL/dW0, dL/dW1, dL/dW2]) as fp64"""
    Fo = F.to(dtype).requires_grad_(True)
    Wo = [w.to(dtype).requires_grad_(True) for w in W]
    out = _apply(kind, Fo, Wo)
    grads = torch.autograd.grad((out * gout.to(dtype)).sum(), [Fo] + Wo)
    return out.detach().double(), grads[0].double(), [g.double() for g in grads[1:]]


def rel(a, b):
    """max-norm relative distance of a from b"""
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


class PrefixRef:
    """out, dL/dF (rows) and dL/dW (sums over the first n rows) of one net for the dense cotangent, for any n <= N_MAX.
    Rows are evaluated in stretches between the counts asked for, each row once; a count's weight gradient is the nearest
    smaller count's plus its stretch.  Every stretch also goes through the oracle in fp32 - the reference's own fp32 run,
    whose distance from the fp64 run (`noise`) says what the input's conditioning costs any fp32 evaluation."""

    def __init__(self, kind, W, with_grad=True):
        self.kind, self.W, self.with_grad = kind, W, with_grad
        self.out = torch.zeros(N_MAX, 3, 3, dtype=torch.float64)
        self.gF = torch.zeros(N_MAX, 3, 3, dtype=torch.float64)
        self.gF32 = torch.zeros(N_MAX, 3, 3, dtype=torch.float64)
        self.rows_done = 0
        self.counts = [0]
        self.dW = {0: [torch.zeros_like(w) for w in W]}
        self.dW32 = {0: [torch.zeros_like(w) for w in W]}

    def _rows(self, n):
        if n > self.rows_done and not self.with_grad:
            with torch.no_grad():
                self.out[self.rows_done:n] = _apply(self.kind, separated_F()[self.rows_done:n], self.W)
            self.rows_done = n

    def get(self, n):
        """with_grad: (out, dL/dF, dL/dW, noise = dict(gF=, dW=[...]) of the fp32 run); else out"""
        if not self.with_grad:
            self._rows(n)
            return self.out[:n]
        if n not in self.dW:
            m = self.counts[bisect.bisect_right(self.counts, n) - 1]
            out, gF, dW = per_rows_ref(self.kind, separated_F()[m:n], dense_gout()[m:n], self.W)
            _, gF32, dW32 = per_rows_ref(self.kind, separated_F()[m:n], dense_gout()[m:n], self.W, torch.float32)
            self.out[m:n], self.gF[m:n], self.gF32[m:n] = out, gF, gF32
            self.dW[n] = [a + d for a, d in zip(self.dW[m], dW)]
            self.dW32[n] = [a + d for a, d in zip(self.dW32[m], dW32)]      # (stretches added in fp64: no more than fp32 costs)
            bisect.insort(self.counts, n)
        noise = dict(gF=rel(self.gF32[:n], self.gF[:n]), dW=[rel(a, d) for a, d in zip(self.dW32[n], self.dW[n])], dW32=self.dW32[n])
        return self.out[:n], self.gF[:n], self.dW[n], noise


def forward_ref(name, kind, n):
    """oracle output of the plain checkpoint `name` on separated_F()[:n]"""
    return _once(("fwd", name, kind), lambda: PrefixRef(kind, weights(name, kind, lora=False), with_grad=False)).get(n)


def dense_ref(kind, n):
    """(out, dL/dF, dL/dW) of jelly + golden LoRA on separated_F()[:n] with dense_gout()[:n]"""
    return _once(("dense", kind), lambda: PrefixRef(kind, weights("jelly", kind, lora=True))).get(n)


def boundary_ref(kind, n):
    """(dL/dF (n, 3, 3), dL/dW, noise) of jelly + golden LoRA with boundary_gout(n): the rows with a cotangent go through the
    oracle, every other row's dL/dF is exactly zero and adds exactly nothing to dL/dW"""
    rows = boundary_rows(n)
    W = weights("jelly", kind, lora=True)
    _, gF_rows, dW = per_rows_ref(kind, separated_F()[rows], boundary_gout(n)[rows], W)
    _, gF32, dW32 = per_rows_ref(kind, separated_F()[rows], boundary_gout(n)[rows], W, torch.float32)
    gF = torch.zeros(n, 3, 3, dtype=torch.float64)
    gF[rows] = gF_rows
    return gF, dW, dict(gF=rel(gF32, gF_rows), dW=[rel(a, d) for a, d in zip(dW32, dW)])


NOISE_CAP = 5e-5      # no bound of this module is wider than 2 x this, whatever the fp32 run of the reference does


def bound(issue, noise):
    """The bound of a backward quantity: the one the suite holds it to at its golden and ragged-tail inputs, or - where the
    inputs of this module are worse conditioned than those - twice the distance of the reference's own fp32 run from its fp64
    run.  The separated inputs stretch a particle by up to 50 % (the golden inputs: 5 %); the jelly net answers with stresses
    of 1e4 .. 6e5 and gradients whose fp32 evaluation by the oracle itself is 0.5e-5 .. 3e-5 from fp64 (dL/dF, dL/dW1): the
    fixed bounds 1e-5 / 2e-5 would ask more of the kernel than the reference delivers.  Two fp32 evaluations of one function
    share the condition number, not the rounding errors: the kernel (its own SVD, its own erf, MFMA accumulation order) is
    allowed twice the reference's fp32 error and no more.  The factor is a judgement, not a theorem; what limits it is the cap:
    the fp32 run's distance counts up to NOISE_CAP only (tests/test_material_edges_cpu.py asserts that it stays below that at
    every count of CASES, so the cap is idle unless torch's fp32 SVD goes wrong somewhere), and no bound exceeds 1e-4 - three
    orders of magnitude below the 1/12 a lost particle costs under a boundary cotangent.  Nothing here comes from the kernel."""
    return max(issue, 2.0 * min(noise, NOISE_CAP))


# ---------------------------------------------------------------- the fused roll-out's counts (tests/test_gpu_rollout_edges.py)
# case: (n, substeps, grid cells per axis, geometry the count is there for)
ROLLOUT_EDGES = {
    "a": (33, 3, 32, dict(grid=1, q=16, last_wave=1, last_tile=1, split=True)),            # waves 0..2 used, wave 3 empty
    "b": (1_991, 3, 32, dict(grid=32, q=16, last_wave=7, split=True)),
    "c": (14_351, 2, 32, dict(grid=225, q=16, last_tile=15, split=False)),                 # unsplit prologue, partial tile
    "d": (16_393, 2, 32, dict(grid=129, q=32, tiles_per_round="2", last_wave=9, split=True)),
    "e": (65_553, 2, 64, dict(grid=205, q=80, tiles_per_round="4 + 1", last_wave=33, split=True)),      # look-ahead across the round boundary
}
