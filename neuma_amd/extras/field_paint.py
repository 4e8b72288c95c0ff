"""Field paint in torch fp64: the CPU path of neuma_amd/field_paint.py (as extras/colliders.py and extras/gaussian_export.py are of
their features) and the yardstick its HIP kernels (csrc/nm_paint.hip, csrc/nm_particle_field.h) are held to.  The definitions, stated
once in include/neuma_hip.h ("field paint") and restated here:

  quantity q per particle, J = det F, tau = elasticity(F) the Kirchhoff stress:
      speed         |v|
      displacement  |x - x0|
      volume        J
      strain        e_i = log(max(|s_i|, 1e-20)), s the singular values of F, m = mean(e), q = sqrt(2/3 sum_i (e_i - m)^2)
      pressure      -tr(tau) / (3 J)                                                             NaN where J <= 0
      von_mises     sigma = (tau + tau^T) / (2 J), d = sigma - tr(sigma)/3 I, q = sqrt(3/2 sum d_ab^2)   NaN where J <= 0
    a NaN or Inf in an array the quantity reads gives NaN.  Non-finite means "no data" below.
  value per Gaussian over the binding CSR (rowptr, col, val):  g_k = (sum_j val_kj q[col_kj]) / (sum_j val_kj);
    NaN for an empty row, a weight sum of 0, a non-finite bound q and a column outside [0, n).
  range [lo, hi], hi > lo: given, or min / max over the finite g; hi <= lo widens to [lo, lo + 1], no finite value gives [0, 1].
  colour  t = clamp((g - lo) / (hi - lo), 0, 1); n knots c_0..c_{n-1} at equal spacing, 2 <= n <= 8:
    i = min(floor(t (n-1)), n-2), u = t (n-1) - i, rgb = c_i + u (c_{i+1} - c_i); a non-finite g takes NODATA.
  output  the SH DC coefficient (rgb - 0.5) / C0 as a (K, 1, 3) feature tensor: rendered at sh_degree 0 the Gaussian shows rgb.
"""
import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ..render.general_utils import C0

QUANTITIES = ("speed", "displacement", "volume", "strain", "pressure", "von_mises")      # index = NM_FIELD_*
NEEDS = {"speed": ("v",), "displacement": ("x", "x0"), "volume": ("F",), "strain": ("F",), "pressure": ("F", "stress"),
         "von_mises": ("F", "stress")}
COLORMAPS = {
    "heat": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (1.0, 1.0, 1.0)),
    "rainbow": ((0.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0)),
    "coolwarm": ((0.23, 0.30, 0.75), (0.87, 0.87, 0.87), (0.71, 0.02, 0.15)),
    "gray": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
}
NODATA = (0.5, 0.5, 0.5)
MAX_KNOTS = 8
STRAIN_FLOOR = 1e-20


def default_colormap(quantity: str) -> str:
    return "coolwarm" if quantity in ("volume", "pressure") else "heat"


def check_quantity(quantity: str) -> str:
    if quantity not in QUANTITIES:
        raise ValueError(f"color_by: unknown quantity {quantity!r}, one of {', '.join(QUANTITIES)} expected")
    return quantity


def knots_of(colormap) -> Tuple[Tuple[float, float, float], ...]:
    """A built-in map by name, or a sequence of 2..8 rgb knots."""
    if isinstance(colormap, str):
        if colormap not in COLORMAPS:
            raise ValueError(f"colormap: unknown map {colormap!r}, one of {', '.join(COLORMAPS)} expected")
        return COLORMAPS[colormap]
    knots = tuple(tuple(float(a) for a in k) for k in colormap)
    if not (2 <= len(knots) <= MAX_KNOTS) or any(len(k) != 3 for k in knots):
        raise ValueError(f"colormap: 2..{MAX_KNOTS} rgb knots expected, got {len(knots)}")
    return knots


def check_range(value_range) -> Optional[Tuple[float, float]]:
    """None (automatic), or (lo, hi) finite with hi > lo."""
    if value_range is None:
        return None
    try:
        lo, hi = (float(a) for a in value_range)
    except (TypeError, ValueError):
        raise ValueError(f"color_range: two numbers LO HI expected, got {value_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"color_range: finite LO < HI expected, got {lo} {hi}")
    return lo, hi


def _rows_finite(*arrays: Tensor) -> Tensor:
    ok = None
    for a in arrays:
        f = torch.isfinite(a.reshape(a.shape[0], -1)).all(dim=1)
        ok = f if ok is None else ok & f
    return ok


def particle_field(quantity: str, x: Optional[Tensor] = None, v: Optional[Tensor] = None, F: Optional[Tensor] = None,
                   stress: Optional[Tensor] = None, x0: Optional[Tensor] = None) -> Tensor:
    """q (N,) in fp64 from the arrays the quantity reads (NEEDS); the others may be None."""
    check_quantity(quantity)
    given = dict(x=x, v=v, F=F, stress=stress, x0=x0)
    ins = []
    for name in NEEDS[quantity]:
        if given[name] is None:
            raise ValueError(f"{quantity} reads {name}: must not be None")
        ins.append(given[name].detach().double())
    ok = _rows_finite(*ins)
    nan = torch.full_like(ok, float("nan"), dtype=torch.float64)
    if quantity == "speed":
        q = ins[0].reshape(-1, 3).norm(dim=1)
    elif quantity == "displacement":
        q = (ins[0].reshape(-1, 3) - ins[1].reshape(-1, 3)).norm(dim=1)
    else:
        Fm = ins[0].reshape(-1, 3, 3)
        Fm = torch.where(ok[:, None, None], Fm, torch.eye(3, dtype=torch.float64, device=Fm.device).expand_as(Fm))
        J = torch.linalg.det(Fm)
        if quantity == "volume":
            q = J
        elif quantity == "strain":
            e = torch.log(torch.linalg.svdvals(Fm).abs().clamp_min(STRAIN_FLOOR))
            q = torch.sqrt(2.0 / 3.0 * ((e - e.mean(dim=1, keepdim=True)) ** 2).sum(dim=1))
        else:
            tau = ins[1].reshape(-1, 3, 3)
            tau = torch.where(ok[:, None, None], tau, torch.zeros_like(tau))
            Jp = torch.where(J > 0, J, torch.ones_like(J))
            tr = tau.diagonal(dim1=1, dim2=2).sum(dim=1)
            if quantity == "pressure":
                q = -tr / (3.0 * Jp)
            else:
                sigma = (tau + tau.transpose(1, 2)) / (2.0 * Jp)[:, None, None]
                d = sigma - (sigma.diagonal(dim1=1, dim2=2).sum(dim=1) / 3.0)[:, None, None] * torch.eye(3, dtype=torch.float64, device=tau.device)
                q = torch.sqrt(1.5 * (d * d).sum(dim=(1, 2)))
            q = torch.where(J > 0, q, nan)
    return torch.where(ok, q, nan)


def gaussian_values(values: Tensor, rowptr: Tensor, col: Tensor, val: Tensor) -> Tensor:
    """g (K,) in fp64 over the CSR rows."""
    q = values.detach().double().reshape(-1)
    n, K = q.numel(), rowptr.numel() - 1
    rp = rowptr.long()
    counts = rp[1:] - rp[:-1]
    rows = torch.repeat_interleave(torch.arange(K, device=q.device), counts)
    c, w = col.long(), val.detach().double()
    inside = (c >= 0) & (c < n)
    qq = torch.where(inside, q[c.clamp(0, max(n - 1, 0))] if n > 0 else torch.zeros_like(w), torch.full_like(w, float("nan")))
    fin = torch.isfinite(qq)
    num = torch.zeros(K, dtype=torch.float64, device=q.device).index_add_(0, rows, torch.where(fin, w * qq, torch.zeros_like(w)))
    den = torch.zeros(K, dtype=torch.float64, device=q.device).index_add_(0, rows, w)
    bad = torch.zeros(K, dtype=torch.float64, device=q.device).index_add_(0, rows, (~fin).double()) > 0
    nodata = bad | (counts == 0) | (den == 0)
    return torch.where(nodata, torch.full_like(den, float("nan")), num / torch.where(den == 0, torch.ones_like(den), den))


def data_range(g: Tensor) -> Tuple[float, float]:
    """The range of the finite values with the widening rule."""
    f = g[torch.isfinite(g)]
    if f.numel() == 0:
        return 0.0, 1.0
    lo, hi = float(f.min()), float(f.max())
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def widen(lo: float, hi: float) -> Tuple[float, float]:
    """The widening rule on a (min, max) pair that may still be the empty pair (+inf, -inf)."""
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        return 0.0, 1.0
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def colors(g: Tensor, value_range: Sequence[float], colormap) -> Tensor:
    """rgb (K, 3) in fp64."""
    knots = torch.tensor(knots_of(colormap), dtype=torch.float64, device=g.device)
    lo, hi = float(value_range[0]), float(value_range[1])
    n = knots.shape[0]
    g = g.detach().double().reshape(-1)
    fin = torch.isfinite(g)
    ok = fin & bool(math.isfinite(lo) and math.isfinite(hi) and hi > lo)
    t = ((torch.where(fin, g, torch.zeros_like(g)) - lo) / (hi - lo if hi != lo else 1.0)).clamp(0.0, 1.0)
    tn = t * (n - 1)
    i = torch.floor(tn).long().clamp(max=n - 2)
    u = (tn - i.double())[:, None]
    rgb = knots[i] + u * (knots[i + 1] - knots[i])
    return torch.where(ok[:, None], rgb, torch.tensor(NODATA, dtype=torch.float64, device=g.device).expand_as(rgb))


def dc_of(rgb: Tensor) -> Tensor:
    """(K, 3) colours -> (K, 1, 3) SH DC coefficients"""
    return ((rgb - 0.5) / C0)[:, None, :]


def paint(values: Tensor, rowptr: Optional[Tensor], col: Optional[Tensor], val: Optional[Tensor], colormap,
          value_range=None) -> Tuple[Tensor, Tensor, Tuple[float, float]]:
    """(shs (K,1,3), g (K,), the range used), all fp64.  rowptr None paints the values themselves."""
    g = values.detach().double().reshape(-1) if rowptr is None else gaussian_values(values, rowptr, col, val)
    rng = check_range(value_range) or data_range(g)
    return dc_of(colors(g, rng, colormap)), g, rng
