"""Shared inputs of the field-paint tests (tests/test_field_paint_cpu.py, tests/test_gpu_field_paint.py): fixed seeds, built once per
process.  Everything a kernel reads is fp32; the fp64 yardstick (neuma_amd/extras/field_paint.py) reads the same fp32 numbers.

particles()   N = 4096 states in blocks:
    general      F = R1 diag(s) R2, s log-uniform in [0.2, 5], random rotations, random stress
    reflected    the same with one s negated (det F < 0)
    identity     F = I exactly
    hydrostatic  a general F with det > 0 and tau = -p J I (J = det of the fp32 F, in fp64)
    uniaxial     F = diag(lambda, 1, 1), lambda in [0.3, 3]
    bad          rows with a NaN or an Inf in each of x, v, F, stress, x0 in turn
csr()         a binding CSR with K = 3000 rows of 0..8 entries over N = 1000 particle values; rows that are empty, rows whose weights
              are all zero, rows that touch a non-finite particle value
color_case()  values whose t lies on knots, between knots, below 0 and above 1 for every built-in map.  The builder asserts, in
              fp64, that no interpolated t lies within 1e-4 of a knot or of 0 / 1: the map's slope jumps there.

BOUNDS: the fp32-against-fp64 error of every quantity measured with the host program (tests/field_paint_host/) on these very inputs,
times about four - the margin that covers the device's v_rsq / v_log / v_sqrt variants of the same arithmetic."""
import functools
import math

import torch

N = 4096
BLOCKS = {"general": (0, 2048), "reflected": (2048, 2560), "identity": (2560, 3072), "hydrostatic": (3072, 3584),
          "uniaxial": (3584, 4056), "bad": (4056, 4096)}
K_CSR, N_CSR = 3000, 1000

# quantity -> bound on max|q32 - q64| over the finite rows, relative to the largest |q64| of the case (measured on the host: the
# figure in the comment; bound = about 4 x).  Nothing here may exceed 1e-5: that would be a defect in the code.
BOUNDS = {
    "speed": 2.7e-7,         # measured 6.7e-8
    "displacement": 3.0e-7,  # measured 7.6e-8
    "volume": 3.2e-7,        # measured 8.0e-8
    "strain": 8.5e-7,        # measured 2.1e-7
    "pressure": 3.5e-7,      # measured 8.6e-8
    "von_mises": 3.7e-7,     # measured 9.3e-8
}
STRAIN_IDENTITY_ABS = 1e-6   # the identity block's strain, absolute (measured 0.0 on the host: 4 x 0 is no bound, so the issue's ceiling)
G_BOUND = 5.6e-7             # the binding-weighted mean, relative to the largest |g64| (measured 1.4e-7: fp32 sums in CSR order, numpy)
COLOR_ABS = 6.2e-7           # a colour through a map, absolute in rgb (measured 1.6e-7, `heat`); far below 1/1020
CSR_COLOR_ABS = 2.1e-6       # a colour of the painted CSR case, absolute in rgb: g's error times the map's slope (measured on the device:
                             # 5.3e-7 `rainbow`, explicit range; 4.3e-7 `heat`, automatic range; 3.4e-7 `coolwarm`, explicit range)
KNOT_CLEARANCE = 1e-4


def _rotations(n, g):
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def _general_F(n, g, negate=False):
    s = torch.exp(math.log(0.2) + (math.log(5.0) - math.log(0.2)) * torch.rand(n, 3, generator=g, dtype=torch.float64))
    if negate:
        s[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] *= -1.0
    return _rotations(n, g) @ torch.diag_embed(s) @ _rotations(n, g)


@functools.lru_cache(maxsize=None)
def particles():
    """dict of fp32 tensors x, v, F, stress, x0 (leave them unchanged), plus fp64 `p` (hydrostatic block) and `lam` (uniaxial block)."""
    g = torch.Generator().manual_seed(20240611)
    x0 = torch.rand(N, 3, generator=g, dtype=torch.float64)
    x = x0 + 0.2 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    v = 3.0 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    F = torch.empty(N, 3, 3, dtype=torch.float64)
    tau = 1e3 * torch.randn(N, 3, 3, generator=g, dtype=torch.float64)
    a, b = BLOCKS["general"]
    F[a:b] = _general_F(b - a, g)
    a, b = BLOCKS["reflected"]
    F[a:b] = _general_F(b - a, g, negate=True)
    a, b = BLOCKS["identity"]
    F[a:b] = torch.eye(3, dtype=torch.float64)
    a, b = BLOCKS["hydrostatic"]
    F[a:b] = _general_F(b - a, g)
    p = 2e3 * (torch.rand(b - a, generator=g, dtype=torch.float64) - 0.5)
    a, b = BLOCKS["uniaxial"]
    lam = torch.exp(math.log(0.3) + (math.log(3.0) - math.log(0.3)) * torch.rand(b - a, generator=g, dtype=torch.float64))
    F[a:b] = torch.eye(3, dtype=torch.float64)
    F[a:b, 0, 0] = lam
    a, b = BLOCKS["bad"]
    F[a:b] = _general_F(b - a, g)
    out = dict(x=x.float(), v=v.float(), F=F.float(), stress=tau.float(), x0=x0.float())
    lam = out["F"][slice(*BLOCKS["uniaxial"]), 0, 0].double()                      # (the fp32 value the kernels see)
    a, b = BLOCKS["hydrostatic"]
    J = torch.linalg.det(out["F"][a:b].double())
    assert bool((J > 0).all())
    tau_h = (-p * J)[:, None, None] * torch.eye(3, dtype=torch.float64)
    out["stress"][a:b] = tau_h.float()
    a, b = BLOCKS["bad"]
    bads = (float("nan"), float("inf"), float("-inf"))
    for i, name in enumerate(("x", "v", "F", "stress", "x0")):                     # 8 rows each, one entry spoiled
        for j in range(8):
            row = a + 8 * i + j
            out[name][row].view(-1)[j % out[name][row].numel()] = bads[j % 3]
    assert bool((torch.linalg.det(out["F"][slice(*BLOCKS["reflected"])].double()) < 0).all())
    out.update(p=p, lam=lam, stress_hydro64=tau_h)
    return out


def bad_rows(quantity):
    """The rows of the `bad` block whose spoiled array the quantity reads"""
    from neuma_amd.extras.field_paint import NEEDS
    a, _ = BLOCKS["bad"]
    rows = []
    for i, name in enumerate(("x", "v", "F", "stress", "x0")):
        if name in NEEDS[quantity]:
            rows += list(range(a + 8 * i, a + 8 * i + 8))
    return rows


@functools.lru_cache(maxsize=None)
def csr():
    """dict: rowptr (K + 1) int32, col, val (fp32), q (N_CSR,) fp32 with some non-finite entries, and the row sets empty, zero_weight,
    touching (lists of row indices)."""
    g = torch.Generator().manual_seed(77)
    counts = torch.randint(0, 9, (K_CSR,), generator=g)
    counts[:40] = 0
    counts[40:80] = torch.randint(1, 9, (40,), generator=g)
    rowptr = torch.zeros(K_CSR + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(counts, 0)
    nnz = int(rowptr[-1])
    col = torch.randint(0, N_CSR, (nnz,), generator=g)
    val = 0.05 + torch.rand(nnz, generator=g)
    q = 10.0 * torch.rand(N_CSR, generator=g) - 2.0
    spoiled = torch.tensor([3, 250, 777, 999])
    q[spoiled] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")])
    for r in range(40, 80):                                                         # all-zero weights
        val[rowptr[r]:rowptr[r + 1]] = 0.0
    rows = torch.repeat_interleave(torch.arange(K_CSR), counts)
    hit = torch.isin(col, spoiled)
    for r in range(100, 110):                                                       # rows made to touch a spoiled particle
        if counts[r] > 0:
            col[rowptr[r]] = spoiled[r % 4]
    hit = torch.isin(col, spoiled)
    touching = sorted(set(rows[hit].tolist()) - set(range(40, 80)))
    empty = [r for r in range(K_CSR) if counts[r] == 0]
    assert len(empty) >= 40 and len(touching) >= 10 and int(counts.max()) == 8
    return dict(rowptr=rowptr.to(torch.int32), col=col.to(torch.int32), val=val.float(), q=q.float(), empty=empty,
                zero_weight=[r for r in range(40, 80)], touching=touching)


def csr_bindings(device):
    """The CSR case as a tune.Bindings on `device` (built from its COO form: Bindings sorts by (row, column))."""
    from neuma_amd.tune import Bindings
    c = csr()
    counts = (c["rowptr"][1:] - c["rowptr"][:-1]).long()
    rows = torch.repeat_interleave(torch.arange(K_CSR), counts)
    return Bindings(torch.stack([rows, c["col"].long()]), c["val"], (K_CSR, N_CSR), device)


@functools.lru_cache(maxsize=None)
def color_case():
    """dict: g (fp32) over the range [lo, hi] = [0, 1] (so t = g), `interp` (bool: strictly between knots), `on_knot`, `outside`."""
    from neuma_amd.extras.field_paint import COLORMAPS
    gen = torch.Generator().manual_seed(5)
    knots = sorted({i / (n - 1) for n in {len(k) for k in COLORMAPS.values()} for i in range(n)})
    between = torch.rand(2000, generator=gen, dtype=torch.float64)
    kt = torch.tensor(knots, dtype=torch.float64)
    between = between[((between[:, None] - kt[None, :]).abs().min(dim=1).values > 4 * KNOT_CLEARANCE)][:1500]
    on = kt.clone()
    outside = torch.tensor([-0.5, -1e-3, -100.0, 1.001, 1.5, 1e6], dtype=torch.float64)
    g = torch.cat([between, on, outside]).float()
    interp = torch.zeros(g.numel(), dtype=torch.bool)
    interp[:between.numel()] = True
    t = g.double()[interp]
    clear = (t[:, None] - kt[None, :]).abs().min(dim=1).values
    assert float(clear.min()) > KNOT_CLEARANCE and float(t.min()) > KNOT_CLEARANCE and float(t.max()) < 1 - KNOT_CLEARANCE
    on_knot = torch.zeros_like(interp)
    on_knot[between.numel():between.numel() + on.numel()] = True
    return dict(g=g, lo=0.0, hi=1.0, interp=interp, on_knot=on_knot, outside=~(interp | on_knot), knots=knots)
