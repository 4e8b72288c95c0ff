"""Colouring a roll-out by stress, strain or speed (no reference counterpart): a per-particle quantity, its binding-weighted mean per
Gaussian, a range and a colour map, as SH DC coefficients the rasterizer renders at sh_degree 0 - on the native kernels of
csrc/nm_paint.hip.  Definition: include/neuma_hip.h ("field paint") and DESIGN.md section 7; the same in torch fp64:
neuma_amd/extras/field_paint.py, which is also what runs for tensors on the CPU.  The rasterizer is untouched.

    particle_field(quantity, x=, v=, F=, stress=, x0=) -> q (N,)
    paint(values, bindings, colormap, value_range=None) -> (shs (K,1,3), g (K,))
    FieldPainter(quantity, colormap, value_range)            what the drivers hold: painter.frame(x, v, F, stress_fn, bindings)

    python -m neuma_amd.render ... --color_by von_mises [--color_range LO HI] [--colormap NAME]
"""
import ctypes as C
import math
from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib as L
from .tune import Bindings

QUANTITIES = ("speed", "displacement", "volume", "strain", "pressure", "von_mises")      # index = NM_FIELD_*
NEEDS = {"speed": ("v",), "displacement": ("x", "x0"), "volume": ("F",), "strain": ("F",), "pressure": ("F", "stress"),
         "von_mises": ("F", "stress")}                                                    # the arrays a quantity reads
COLORMAPS = {                                                                            # rgb knots at equal spacing
    "heat": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (1.0, 1.0, 1.0)),
    "rainbow": ((0.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0)),
    "coolwarm": ((0.23, 0.30, 0.75), (0.87, 0.87, 0.87), (0.71, 0.02, 0.15)),
    "gray": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
}
NODATA = (0.5, 0.5, 0.5)
MAX_KNOTS = 8               # NM_PAINT_MAX_KNOTS


def _extras():
    """the fp64 definition: what runs for tensors on the CPU (the GPU path imports none of it)"""
    from .extras import field_paint
    return field_paint


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


def widen(lo: float, hi: float) -> Tuple[float, float]:
    """The widening rule on a (min, max) pair that may still be the empty pair (+inf, -inf)."""
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        return 0.0, 1.0
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def _f32(t: Tensor, n: int, tail: Tuple[int, ...], name: str) -> Tensor:
    if t.numel() != n * math.prod(tail):
        raise ValueError(f"{name}: shape ({n}, {', '.join(map(str, tail))}) expected, got {tuple(t.shape)}")
    return t.detach().float().reshape(n, *tail).contiguous()


def particle_field(quantity: str, x: Optional[Tensor] = None, v: Optional[Tensor] = None, F: Optional[Tensor] = None,
                   stress: Optional[Tensor] = None, x0: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """q (N,) fp32 of the particles; only the arrays the quantity reads (NEEDS) are needed.  GPU tensors go
    through nm_particle_field, CPU tensors through the fp64 definition (returned as fp32)."""
    check_quantity(quantity)
    given = dict(x=x, v=v, F=F, stress=stress, x0=x0)
    read = {k: given[k] for k in NEEDS[quantity]}
    for k, t in read.items():
        if t is None:
            raise ValueError(f"{quantity} reads {k}: must not be None")
    first = next(iter(read.values()))
    if not first.is_cuda:
        return _extras().particle_field(quantity, **read).float()
    dev = L.same_device(*read.values())
    n = first.shape[0]
    tails = dict(x=(3,), v=(3,), x0=(3,), F=(3, 3), stress=(3, 3))
    a = {k: _f32(t, n, tails[k], k) for k, t in read.items()}
    q = out if out is not None else torch.empty(n, dtype=torch.float32, device=dev)
    if q.numel() != n:
        raise ValueError(f"out: {n} values expected")
    L.check(L.lib().nm_particle_field(n, QUANTITIES.index(quantity), L.ptr(a.get("x")), L.ptr(a.get("v")), L.ptr(a.get("F")),
                                      L.ptr(a.get("stress")), L.ptr(a.get("x0")), L.ptr(q, torch.float32), L.stream_ptr(dev)),
            "nm_particle_field")
    return q


def field_range(g: Tensor, out: Optional[Tensor] = None, fold: bool = False) -> Tensor:
    """nm_field_range on a GPU tensor g (K,): 2 device floats {lo, hi}, no read-back.  fold=False writes the range of g with the
    widening rule; fold=True folds g's finite min / max into `out` (start it with empty_range)."""
    g = g.detach().float().contiguous().reshape(-1)
    if out is None:
        if fold:
            raise ValueError("field_range: fold needs the running pair in `out`")
        out = torch.empty(2, dtype=torch.float32, device=g.device)
    lib = L.lib()
    k = g.numel()
    nws = int(lib.nm_field_range_workspace(k))
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=g.device)
    L.check(lib.nm_field_range(k, L.ptr(g), L.ptr(out, torch.float32), 1 if fold else 0, L.ptr(ws), nws, L.stream_ptr(g.device)),
            "nm_field_range")
    return out


def empty_range(device) -> Tensor:
    """The running pair before its first frame: {+inf, -inf}"""
    return torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device=device)


def _csr(bindings):
    return None if bindings is None else Bindings.of(bindings)


def paint_raw(values: Tensor, bindings, colormap=None, range_dev: Optional[Tensor] = None, want_g: bool = True,
              g_out: Optional[Tensor] = None, dc_out: Optional[Tensor] = None, want_dc: bool = True):
    """One nm_field_paint launch on GPU tensors: (dc (K,3) or None, g (K,) or None).  range_dev: 2 device floats, needed with want_dc."""
    q = values.detach().float().contiguous().reshape(-1)
    dev, n = q.device, q.numel()
    b = _csr(bindings)
    K = n if b is None else b.K
    if b is not None and b.N != n:
        raise ValueError(f"paint: {n} particle values for bindings over {b.N} particles")
    if want_g and g_out is None:
        g_out = torch.empty(K, dtype=torch.float32, device=dev)
    if want_dc and dc_out is None:
        dc_out = torch.empty(K, 3, dtype=torch.float32, device=dev)
    knots, nk, nod = None, 0, None
    if dc_out is not None:
        kn = knots_of(colormap)
        nk = len(kn)
        knots = (C.c_float * (3 * nk))(*[a for k in kn for a in k])
        nod = (C.c_float * 3)(*NODATA)
        if range_dev is None or range_dev.numel() != 2:
            raise ValueError("paint: range_dev (2 device floats) is needed to colour")
    L.check(L.lib().nm_field_paint(K, n, L.ptr(b.rowptr) if b is not None else None, L.ptr(b.col) if b is not None else None,
                                   L.ptr(b.val) if b is not None else None, L.ptr(q), L.ptr(range_dev, torch.float32) if dc_out is not None else None,
                                   nk, knots, nod, L.ptr(g_out), L.ptr(dc_out), L.stream_ptr(dev)), "nm_field_paint")
    return dc_out, g_out


def paint(values: Tensor, bindings, colormap="heat", value_range=None) -> Tuple[Tensor, Tensor]:
    """(shs (K,1,3), g (K,)) fp32: the particle values (N,) averaged over each Gaussian's bound particles and mapped to colours.
    bindings: tune.Bindings (or a sparse K x N tensor), or None to paint the values themselves (K = N).  value_range: (lo, hi), or
    None for the range of the data (found on the device: no read-back either way).  CPU tensors take the fp64 definition."""
    knots_of(colormap)
    rng = check_range(value_range)
    if not values.is_cuda:
        b = _csr(bindings)
        shs, g, _ = _extras().paint(values, *((None, None, None) if b is None else (b.rowptr.cpu(), b.col.cpu(), b.val.cpu())), colormap, rng)
        return shs.float(), g.float()
    if rng is not None:
        r = torch.tensor(rng, dtype=torch.float32, device=values.device)
        dc, g = paint_raw(values, bindings, colormap, r)
    else:
        _, g = paint_raw(values, bindings, want_dc=False)
        r = field_range(g)
        dc, _ = paint_raw(g, None, colormap, r, want_g=False)
    return dc[:, None, :], g


class FieldPainter(object):
    """What a driver holds for --color_by: the quantity, the map, the explicit or automatic range, the running overall range on the
    device and which inputs the quantity reads.  `frame` returns the painted coefficients of one frame; nothing is read back
    before `overall_range`."""

    def __init__(self, quantity: str, colormap: Optional[str] = None, value_range=None, x0: Optional[Tensor] = None):
        self.quantity = check_quantity(quantity)
        self.colormap = colormap if colormap is not None else default_colormap(quantity)
        knots_of(self.colormap)
        self.value_range = check_range(value_range)
        self.needs = NEEDS[quantity]
        self.x0 = x0                    # displacement: the positions it is measured from (default: those of the first frame)
        self.running = None             # device {min, max} over the frames so far (automatic range only)
        self.last_q = None              # the last frame's particle values (N,) and Gaussian values (K,)
        self.last_g = None
        self._range_dev = None

    @property
    def automatic(self) -> bool:
        return self.value_range is None

    @property
    def frame_range(self) -> Optional[Tensor]:
        """The range the last frame was painted with: 2 device floats {lo, hi} (None before the first GPU frame)."""
        return self._range_dev

    def describe(self) -> str:
        if self.automatic:
            return (f"color_by {self.quantity} ({self.colormap}): no --color_range, every frame is scaled by its own range "
                    "(the sequence's overall range is printed at the end)")
        return f"color_by {self.quantity} ({self.colormap}): range {self.value_range[0]:g} .. {self.value_range[1]:g}"

    def values(self, x: Tensor, v: Tensor, F: Tensor, stress_fn: Optional[Callable[[Tensor], Tensor]]) -> Tensor:
        """The frame's particle values: one elasticity call where the quantity reads the stress, none otherwise."""
        if "x0" in self.needs and self.x0 is None:
            self.x0 = x.detach().clone()
        stress = None
        if "stress" in self.needs:
            if stress_fn is None:
                raise ValueError(f"{self.quantity} reads the stress: stress_fn is needed")
            stress = stress_fn(F)
        given = dict(x=x, v=v, F=F, stress=stress, x0=self.x0)
        self.last_q = particle_field(self.quantity, **{k: given[k] for k in self.needs})
        return self.last_q

    def frame(self, x: Tensor, v: Tensor, F: Tensor, stress_fn, bindings: Union[object, Sequence],
              sections: Optional[Sequence[int]] = None) -> Tensor:
        """shs (K,1,3) of this frame.  bindings: one binding matrix, or one per object with `sections` = the objects' particle counts;
        each object's rows are painted through its own bindings and the range is shared."""
        q = self.values(x, v, F, stress_fn)
        blist = list(bindings) if isinstance(bindings, (list, tuple)) else [bindings]
        secs = [q.numel()] if sections is None else [int(s) for s in sections]
        if len(secs) != len(blist) or sum(secs) != q.numel():
            raise ValueError(f"frame: {len(blist)} binding matrices, sections {secs} for {q.numel()} particles")
        bs = [Bindings.of(b) for b in blist]
        if not q.is_cuda:
            gs = [_extras().gaussian_values(qq, b.rowptr.cpu(), b.col.cpu(), b.val.cpu()) for qq, b in zip(torch.split(q, secs), bs)]
            g = torch.cat(gs)
            rng = self.value_range or _extras().data_range(g)
            if self.automatic:
                f = g[torch.isfinite(g)]
                lo, hi = self.running if self.running is not None else (float("inf"), float("-inf"))
                if f.numel():
                    lo, hi = min(lo, float(f.min())), max(hi, float(f.max()))
                self.running = (lo, hi)
            self.last_g = g.float()
            return _extras().dc_of(_extras().colors(g, rng, self.colormap)).float()
        dev = q.device
        K = sum(b.K for b in bs)
        g = torch.empty(K, dtype=torch.float32, device=dev)
        offs, o = [], 0
        for b in bs:
            offs.append(o)
            o += b.K
        qparts = torch.split(q, secs)
        if self.automatic:
            if self.running is None:
                self.running = empty_range(dev)
                self._range_dev = torch.empty(2, dtype=torch.float32, device=dev)
            for qq, b, o in zip(qparts, bs, offs):
                paint_raw(qq, b, want_dc=False, g_out=g[o:o + b.K])
            field_range(g, self._range_dev)
            field_range(g, self.running, fold=True)
            dc, _ = paint_raw(g, None, self.colormap, self._range_dev, want_g=False)
        else:
            if self._range_dev is None:
                self._range_dev = torch.tensor(self.value_range, dtype=torch.float32, device=dev)
            dc = torch.empty(K, 3, dtype=torch.float32, device=dev)
            for qq, b, o in zip(qparts, bs, offs):
                paint_raw(qq, b, self.colormap, self._range_dev, g_out=g[o:o + b.K], dc_out=dc[o:o + b.K])
        self.last_g = g
        return dc[:, None, :]

    def overall_range(self) -> Optional[Tuple[float, float]]:
        """The sequence's overall range with the widening rule (automatic range only: the one read-back), else the given one."""
        if not self.automatic:
            return self.value_range
        if self.running is None:
            return None
        lo, hi = (float(a) for a in (self.running.cpu() if torch.is_tensor(self.running) else self.running))
        return widen(lo, hi)

    def summary(self) -> Optional[str]:
        r = self.overall_range()
        if not self.automatic or r is None:
            return None
        return (f"color_by {self.quantity}: overall range {r[0]:.9g} .. {r[1]:.9g}; pass --color_range {r[0]:.9g} {r[1]:.9g} "
                "for a steady scale")


def painter_from_cfg(cfg, section=None) -> Optional[FieldPainter]:
    """The painter a driver's config asks for, or None: `color_by` (with `color_range`, `colormap`) from the command line, else from
    `section` (the config section the driver's other render keys live in)."""
    def get(key):
        val = cfg.get(key)
        return val if val is not None or section is None else section.get(key)
    quantity = get("color_by")
    if quantity is None:
        return None
    rng = get("color_range")
    return FieldPainter(str(quantity), get("colormap"), None if rng is None else list(rng))


def painted_gaussians(model, shs: Tensor):
    """`model` (a frame as export.deformed_gaussians makes it) with the painted DC colour and no rest coefficients: a degree-0 3DGS
    parameter set any viewer shows the field with."""
    from .render.gaussian_model import GaussianModel
    K = model._xyz.shape[0]
    if tuple(shs.shape) != (K, 1, 3):
        raise ValueError(f"shs must be ({K}, 1, 3), got {tuple(shs.shape)}")
    out = GaussianModel(0)
    return out.set_params(model._xyz, shs.detach().contiguous(), shs.new_zeros(K, 0, 3), model._scaling, model._rotation, model._opacity)


def save_particles_ply(path, points: Tensor, values: Tensor, quantity: str) -> None:
    """The particle file of --save_particles with a fourth float property named after the quantity."""
    import numpy as np
    from .io import write_ply_vertices
    pts = points.detach().float().cpu().numpy().reshape(-1, 3)
    write_ply_vertices(path, ["x", "y", "z", quantity], np.concatenate([pts, values.detach().float().cpu().numpy().reshape(-1, 1)], axis=1))
