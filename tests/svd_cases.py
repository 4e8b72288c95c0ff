"""Input families, fp64 yardstick and error metrics for the 3x3 SVD (nm_svd3) and its consumers.  A plain helper module shared by
tests/test_svd_host_cpu.py (host half of nm_svd3, no GPU) and tests/test_gpu_svd_edges.py (the device kernels).

Matrices are composed in fp64 as Ru diag(s) Rv^T with Haar rotations and rounded to fp32 ONCE; the yardstick
(oracle.material.svd3 in fp64) always works on the rounded values, so it sees exactly what the kernel sees."""
from collections import OrderedDict
from itertools import permutations, product

import torch

from oracle import material as om

MAX_ROWS = 1000
# families whose determinant is non-zero by construction: the rule sign(sigma_2) == sign(det F) is checked on these
FULL_RANK = ("cond1e3", "cond1e6", "tie01", "tie12", "tie1m2", "tie012", "rotations", "near_tie", "perm_refl")
SCALED_IN_EXPONENTS = (-30, -20, 20, 27)
SCALED_OUT_EXPONENTS = (-100, -60, -40, 34, 50, 60)
# families the fused constitutive nets are run on (`scaled_in` only with the exponents +-20)
NET_FAMILIES = ("baseline", "cond1e3", "tie01", "tie12", "tie1m2", "tie012", "near_tie", "rotations", "scaled_in")
NET_SCALED_IN_EXPONENTS = (-20, 20)
# The nets' outputs go through the polar factor R = U Vh, whose condition is 1 / (s1 + s2): they are compared with fp64 on
# rows with (s1 + s2) >= 0.05 s0 only, and the filter must keep at least this share of each family: 90 %, except where
# the DEFINITION of the family puts rows at s1 + s2 = 0 -
#   tie1m2: s1 = -s2 on every row, nothing can be kept (outputs must be finite there);
#   tie012: the -c R half has sigma = (c, c, -c); exactly the c R half is kept;
#   cond1e3: three log-uniform values over three decades, sorted, half with s2 negated.  With x = log10 s, 0.05 s0 is 1.3
#     decades below s0: a row is dropped when s1 is further below (probability (1 - 1.3 / 3)^3 = 0.18 for the gap between the
#     two largest of three uniform values) or, in the negated half, when s1 - |s2| < 0.05 s0.  400 000 draws keep 78.3 %;
#     the floor is 6 standard deviations of a 1000-row sample below that.
POLAR_KEEP_FLOOR = {name: 0.9 for name in NET_FAMILIES}
POLAR_KEEP_FLOOR.update(tie1m2=0.0, tie012=0.5, cond1e3=0.70)
METRIC_KEYS = ("recon", "orth_U", "orth_V", "det_U", "det_V", "order", "sigma")


def _haar(n, g):
    """n rotations distributed by the Haar measure on SO(3): QR of a Gaussian matrix with the signs of diag(R) fixed."""
    Q, R = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    Q = Q * torch.sign(torch.diagonal(R, dim1=1, dim2=2))[:, None, :]
    Q[:, :, 2] *= torch.sign(torch.linalg.det(Q))[:, None]
    return Q


def _compose(s, g):
    n = s.shape[0]
    return _haar(n, g) @ torch.diag_embed(s) @ _haar(n, g).transpose(1, 2)


def _loguniform(n, lo, hi, g, cols=None):
    shape = (n,) if cols is None else (n, cols)
    return 10.0 ** (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64))


def _baseline(n, g):
    return torch.eye(3, dtype=torch.float64) + 0.3 * torch.randn(n, 3, 3, generator=g, dtype=torch.float64)


def _cond(n, half_width, g):
    s = torch.sort(_loguniform(n, -half_width, half_width, g, 3), dim=1, descending=True).values
    s[1::2, 2] *= -1.0
    return _compose(s, g)


def families(seed=0):
    """name -> float32 (n, 3, 3), n <= MAX_ROWS, in a fixed order."""
    g = torch.Generator().manual_seed(seed)
    n = MAX_ROWS
    fam = OrderedDict()
    fam["baseline"] = _baseline(n, g)
    fam["cond1e3"] = _cond(n, 1.5, g)
    fam["cond1e6"] = _cond(n, 3.0, g)
    a = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)                     # [1, 2)
    b = a * (0.2 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64))        # [0.2 a, 0.8 a)
    sgn = torch.ones(n, dtype=torch.float64); sgn[3::4] = -1.0
    fam["tie01"] = _compose(torch.stack([a, a, b * sgn], 1), g)                  # s0 = s1, a quarter with det < 0
    fam["tie12"] = _compose(torch.stack([a, b, b], 1), g)                        # s1 = s2
    fam["tie1m2"] = _compose(torch.stack([a, b, -b], 1), g)                      # s1 = -s2
    c = _loguniform(n, -1.0, 1.0, g)
    c[1::2] *= -1.0
    fam["tie012"] = c[:, None, None] * _haar(n, g)                               # c R and -c R
    fam["rotations"] = _haar(n, g)
    eps = _loguniform(n, -7.0, -3.0, g)
    one = torch.ones(n, dtype=torch.float64)
    fam["near_tie"] = _compose(torch.stack([one + eps, one, one - eps], 1), g)
    fam["rank2"] = _compose(torch.stack([a, b, torch.zeros(n, dtype=torch.float64)], 1), g)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    fam["rank1"] = u[:, :, None] * v[:, None, :]
    fam["zero"] = torch.zeros(64, 3, 3, dtype=torch.float64)
    rows = []
    for cc in (1.0, -1.0, 0.37, -2.5e3, 3e-4):
        for i in range(9):
            m = torch.zeros(9, dtype=torch.float64); m[i] = cc
            rows.append(m.view(3, 3))
    fam["single_entry"] = torch.stack(rows)
    zc = _baseline(300, g)
    for k in range(3):
        zc[k::3, :, k] = 0.0
    fam["zero_column"] = zc
    eye = torch.eye(3, dtype=torch.float64)
    perms = [eye[list(p)] for p in permutations(range(3))]
    refl = [torch.diag(torch.tensor(d, dtype=torch.float64)) for d in product((1.0, -1.0), repeat=3)]
    fam["perm_refl"] = torch.stack(perms + [-p for p in perms] + refl)
    fam["diag_unsorted"] = torch.stack([torch.diag(torch.tensor(p, dtype=torch.float64)) for p in permutations((0.5, 1.0, 2.0))]
                                       + [torch.ones(3, 3, dtype=torch.float64)])
    k = n // len(SCALED_IN_EXPONENTS)
    fam["scaled_in"] = torch.cat([_baseline(k, g) * 2.0 ** e for e in SCALED_IN_EXPONENTS])
    k = n // len(SCALED_OUT_EXPONENTS)
    fam["scaled_out"] = torch.cat([_baseline(k, g) * 2.0 ** e for e in SCALED_OUT_EXPONENTS])
    out = OrderedDict((name, F.float().contiguous()) for name, F in fam.items())
    assert all(F.shape[0] <= MAX_ROWS and bool(torch.isfinite(F).all()) for F in out.values())
    return out


def scaled_in_rows(exponents):
    """row mask of the `scaled_in` family for a subset of its exponents"""
    k = MAX_ROWS // len(SCALED_IN_EXPONENTS)
    mask = torch.zeros(k * len(SCALED_IN_EXPONENTS), dtype=torch.bool)
    for i, e in enumerate(SCALED_IN_EXPONENTS):
        if e in exponents:
            mask[i * k:(i + 1) * k] = True
    return mask


def yardstick(F32):
    """fp64 U, sigma, Vh of the fp32-rounded input (project convention: U, V in SO(3), sign on sigma_2) and the polar factor."""
    U, s, Vh = om.svd3(F32.detach().cpu().double())
    return {"U": U, "s": s, "Vh": Vh, "R": U @ Vh}


def metrics(F, U, s, Vh, yard=None):
    """Per-row errors of a decomposition of F, relative to the fp64 sigma_max of that row (absolute where sigma_max == 0):
    recon |U diag(s) Vh - F|max, orth_U |U^T U - I|max, orth_V |Vh Vh^T - I|max, det_U |det U - 1|, det_V |det Vh - 1|,
    order max(s1 - s0, |s2| - s1, 0), sigma |s - s64|max; and sign_ok: sign(s2) == sign(det F) (meaningful on FULL_RANK only).
    orth and det are properties of unit-scale matrices and are not divided by sigma_max."""
    Fd = F.detach().cpu().double()
    U, s, Vh = U.detach().cpu().double(), s.detach().cpu().double(), Vh.detach().cpu().double()
    yard = yardstick(F) if yard is None else yard
    s64 = yard["s"]
    smax = s64[:, 0].clone()
    smax[smax == 0] = 1.0
    I = torch.eye(3, dtype=torch.float64)
    zero = torch.zeros_like(smax)
    return {
        "recon": (U @ torch.diag_embed(s) @ Vh - Fd).abs().amax((1, 2)) / smax,
        "orth_U": (U.transpose(1, 2) @ U - I).abs().amax((1, 2)),
        "orth_V": (Vh @ Vh.transpose(1, 2) - I).abs().amax((1, 2)),
        "det_U": (torch.linalg.det(U) - 1.0).abs(),
        "det_V": (torch.linalg.det(Vh) - 1.0).abs(),
        "order": torch.maximum(torch.maximum(s[:, 1] - s[:, 0], s[:, 2].abs() - s[:, 1]), zero) / smax,
        "sigma": (s - s64).abs().amax(1) / smax,
        "sign_ok": torch.sign(s[:, 2]) == torch.sign(torch.linalg.det(Fd)),
    }


def noise(F32, yard=None):
    """The same metrics for oracle.material.svd3 run in fp32 on the CPU: the reference path's own fp32 error."""
    U, s, Vh = om.svd3(F32.detach().cpu().float())
    return metrics(F32, U, s, Vh, yard)


def worst(m):
    """family-wide maxima of the error metrics; a NaN anywhere gives inf (max() would hide it)"""
    out = {}
    for k in METRIC_KEYS:
        out[k] = float(m[k].max()) if bool(torch.isfinite(m[k]).all()) else float("inf")
    return out


def polar_defined(yard, frac=0.05):
    """rows whose polar factor R = U Vh is well defined: its condition is 1 / (s1 + s2)"""
    s = yard["s"]
    return (s[:, 1] + s[:, 2]) >= frac * s[:, 0]


def gap_separated(yard, frac=0.05):
    s = yard["s"]
    return torch.minimum(s[:, 0] - s[:, 1], s[:, 1] - s[:, 2].abs()) > frac * s[:, 0]
