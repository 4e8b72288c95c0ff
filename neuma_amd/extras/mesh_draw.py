"""Drawing mesh (field) colliders in renders, as torch functions on the CPU: the DEFINITION the native kernels k_field_cast /
k_field_hide (csrc/nm_draw.hip, csrc/nm_field_ray.h) are held to, and the CPU path of neuma_amd.collider_draw.cast_field /
front_opacity_field.  The prose is in include/neuma_hip.h ("Drawing mesh colliders") and DESIGN.md section 7; in short

    drawn solid   {phi < 0} of the trilinearly interpolated field (extras/colliders.py field_phi_normal), cut by the lattice box
                  [origin, origin + (dims - 1) spacing] and by the unit cube
    rays          those of extras/collider_draw.py: o_s = (o_r - b) / a, un-normalised d_s = d_r / a, L = |d_s|
    interval      [t0, t1] = t >= 0, the cube's three slabs, the lattice's three slabs (of equal entries the first stays)
    face hit      phi(t0) < 0: at t0, with that slab's normal; t0 = 0: the camera is inside, the normal faces it
    march         at most STEPS = 192 times: phi <= tau = 1e-3 spacing -> converged; else t += max(phi, tau) / L; a miss once
                  t >= t_end = min(t1, the t already in the buffer)
    polish        three Newton steps along the ray, t -= phi / (grad . d_s), each only while grad . d_s < 0, t kept in [t0, t1]
    shade         color (0.35 + 0.65 max(0, n_r . -d_r)), n_r = normalize(n_s / a), n_s = grad / |grad| (+x where it vanishes)
    merge         in-out on the analytic cast's t / shade / hit: a field hit replaces a pixel only where its t is strictly smaller
    hidden        the same march on the segment camera -> mean (t_end = min(t1, 1)) hits, or the mean lies inside the solid

Everything is evaluated in `dtype`: fp64 is the yardstick; fp32 spells the kernels' operations in the kernels' order, and its
distance from fp64 is what the kernels' own distance is measured against.  phi, origin and spacing are the fp32 values the
kernels read, in either case.  With `margins=True` the fp64 evaluation also returns which pixels / Gaussians sit so close to a
branch that fp32 may decide otherwise (UNSURE, below).  `step_factor` and `max_steps` exist for the no-overshoot check of the
tests (a march with 1/8 of the step); the definition is step_factor = 1, max_steps = STEPS.  Not differentiated."""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import collider_draw as X
from .colliders import field_phi_normal

STEPS = 192
TAU = 1e-3                 # convergence threshold, in lattice spacings
# the unsure set
GRAZE = 0.05               # hits with -n . d / L below this
NEAR_MISS = 0.05           # misses whose smallest phi along the ray is below this many spacings
CAP_MARGIN = 8             # rays that took more than STEPS - CAP_MARGIN steps
T_MARGIN = 1e-4            # t within this (relative) of a competing collider's t; entry ties; a nearly empty interval
FACE_MARGIN = 1e-4         # |phi(t0)| below this many spacings: face hit or march
SEGMENT_MARGIN = 1e-5      # |u_hit - 1|, |phi(mean)|
_INF = float("inf")


class _Field:
    """One FieldCollider's constants in `dtype` (from the fp32 values the C ABI carries)."""

    def __init__(self, c, dtype):
        phi = c.phi.detach().cpu() if torch.is_tensor(c.phi) else torch.from_numpy(np.asarray(c.phi))
        self.f = phi.float().to(dtype).reshape(-1)
        self.origin = [torch.tensor(float(np.float32(v)), dtype=dtype) for v in c.origin]
        self.h = torch.tensor(float(np.float32(c.spacing)), dtype=dtype)
        self.dims = tuple(int(v) for v in c.dims)
        self.hi = [self.origin[a] + torch.tensor(float(self.dims[a] - 1), dtype=dtype) * self.h for a in range(3)]
        self.tau = torch.tensor(TAU, dtype=torch.float32).to(dtype) * self.h


def sample(fld: _Field, o: Tensor, d: Tensor, t: Tensor, want_g: bool = False):
    """phi at o + t d [, the gradient of the interpolant per cell (M,3)]: field_sample of csrc/nm_field_ray.h.  The cell index is
    clamped to 0 .. dims - 2 on both sides."""
    dt = d.dtype
    fr, ii = [], []
    for a in range(3):
        p = o[a] + t * d[:, a]
        q = (p - fld.origin[a]) / fld.h
        top = torch.tensor(float(fld.dims[a] - 2), dtype=dt)
        f = torch.clamp(torch.clamp(torch.floor(q), max=float(top)), min=0.0)
        f = torch.where(torch.isnan(q), top.expand_as(f), f)
        ii.append(f.long())
        fr.append(q - f)
    sy = fld.dims[2]
    sx = fld.dims[1] * sy
    base = ii[0] * sx + ii[1] * sy + ii[2]
    F = fld.f
    f000, f001, f010, f011 = F[base], F[base + 1], F[base + sy], F[base + sy + 1]
    f100, f101, f110, f111 = F[base + sx], F[base + sx + 1], F[base + sx + sy], F[base + sx + sy + 1]
    d00, d01, d10, d11 = f001 - f000, f011 - f010, f101 - f100, f111 - f110
    a00, a01, a10, a11 = f000 + fr[2] * d00, f010 + fr[2] * d01, f100 + fr[2] * d10, f110 + fr[2] * d11
    e0, e1 = a01 - a00, a11 - a10
    b0, b1 = a00 + fr[1] * e0, a10 + fr[1] * e1
    gx = b1 - b0
    phi = b0 + fr[0] * gx
    if not want_g:
        return phi
    gy = e0 + fr[0] * (e1 - e0)
    z0, z1 = d00 + fr[1] * (d01 - d00), d10 + fr[1] * (d11 - d10)
    gz = z0 + fr[0] * (z1 - z0)
    return phi, torch.stack([gx, gy, gz], dim=-1)


def trace(c, o: Tensor, d: Tensor, t_cap: Tensor, want_n: bool = True, step_factor: float = 1.0, max_steps: int = STEPS,
          info: bool = False):
    """field_trace of csrc/nm_field_ray.h for the rays o + t d (o (3,), d (M,3), t_cap (M,), one dtype): hit (M,) bool, t (M,),
    which (M,) int64 (-1: t0 = 0; 0..2 / 3..5: the cube's / the lattice's slab that gave t0; 6: the surface), n (M,3) the outward
    normal in simulation coordinates [, a dict: t0, t1, second (the largest entry among the other constraints), phi0, steps, min_phi
    (over the samples of the march), valid (a non-empty interval)].  Without want_n, t is the march's own (not polished) and n is 0."""
    dt, M = d.dtype, d.shape[0]
    fld = _Field(c, dt)
    zero, one = torch.tensor(0.0, dtype=dt), torch.tensor(1.0, dtype=dt)
    L = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    t0 = torch.zeros(M, dtype=dt)
    t1 = torch.full((M,), _INF, dtype=dt)
    second = torch.full((M,), -_INF, dtype=dt)
    which = torch.full((M,), -1, dtype=torch.int64)
    for k in range(6):
        a = k % 3
        s0, s1 = X._slab(o[a], d[:, a], zero if k < 3 else fld.origin[a], one if k < 3 else fld.hi[a])
        better = s0 > t0
        second = torch.where(better, t0, torch.maximum(second, s0))
        t0 = torch.where(better, s0, t0)
        which = torch.where(better, torch.full_like(which, k), which)
        t1 = torch.minimum(t1, s1)
    t_end = torch.minimum(t1, t_cap)
    valid = t0 < t_end
    phi0 = torch.full((M,), _INF, dtype=dt)
    vi = torch.nonzero(valid)[:, 0]
    phi0[vi] = sample(fld, o, d[vi], t0[vi])
    face = valid & (phi0 < 0)
    ax = torch.where(which < 3, which, which - 3).clamp(min=0)
    dq = torch.gather(d, 1, ax[:, None])[:, 0]
    sg = torch.where(dq > 0, -torch.ones_like(dq), torch.ones_like(dq))
    n = torch.zeros(M, 3, dtype=dt)
    n[face] = torch.nn.functional.one_hot(ax[face], 3).to(dt) * sg[face][:, None]
    # the march
    t, phi = t0.clone(), phi0.clone()
    conv = torch.zeros(M, dtype=torch.bool)
    steps = torch.zeros(M, dtype=torch.int64)
    min_phi = phi0.clone()
    idx = torch.nonzero(valid & ~face)[:, 0]
    for _ in range(max_steps):
        if idx.numel() == 0:
            break
        ph = phi[idx]
        done = ph <= fld.tau
        conv[idx[done]] = True
        idx, ph = idx[~done], ph[~done]
        step = torch.maximum(ph, fld.tau)
        if step_factor != 1.0:
            step = step * step_factor
        tn = t[idx] + step / L[idx]
        t[idx] = tn
        steps[idx] += 1
        idx = idx[~(tn >= t_end[idx])]
        phi[idx] = sample(fld, o, d[idx], t[idx])
        min_phi[idx] = torch.minimum(min_phi[idx], phi[idx])
    ci = torch.nonzero(conv)[:, 0]
    if want_n and ci.numel():
        dc, tc = d[ci], t[ci]
        for _ in range(3):
            ph, g = sample(fld, o, dc, tc, want_g=True)
            gd = (g[:, 0] / fld.h) * dc[:, 0] + (g[:, 1] / fld.h) * dc[:, 1] + (g[:, 2] / fld.h) * dc[:, 2]
            go = gd < 0
            new = torch.minimum(torch.maximum(tc - ph / torch.where(go, gd, torch.ones_like(gd)), t0[ci]), t1[ci])
            tc = torch.where(go, new, tc)
        _, g = sample(fld, o, dc, tc, want_g=True)
        l2 = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]
        length = torch.sqrt(torch.where(l2 > 0, l2, torch.ones_like(l2)))
        ex = torch.tensor([1.0, 0.0, 0.0], dtype=dt).expand_as(g)
        n[ci] = torch.where((l2 > 0)[:, None], g / length[:, None], ex)
        t[ci] = tc
        which = which.clone()
        which[ci] = 6
    hit = face | conv
    t = torch.where(hit, t, torch.full_like(t, _INF))
    if info:
        return hit, t, which, n, dict(t0=t0, t1=t1, second=second, phi0=phi0, steps=steps, min_phi=min_phi, valid=valid, L=L,
                                      spacing=float(fld.h))
    return hit, t, which, n


def _unsure_rays(hit, t, which, n, d, nfo, max_steps: int = STEPS) -> Tensor:
    """The rays of one trace whose decision fp32 may take otherwise, from the fp64 values (module constants)."""
    h = nfo["spacing"]
    ndl = -(n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1] + n[:, 2] * d[:, 2]) / nfo["L"]
    u = hit & (which >= 0) & (ndl < GRAZE)                                                    # grazing hits
    u |= nfo["valid"] & ~hit & (nfo["min_phi"] < NEAR_MISS * h)                               # near misses
    u |= nfo["steps"] > max_steps - CAP_MARGIN                                                # at the cap
    u |= X._close(nfo["t0"], nfo["t1"], T_MARGIN)                                             # a nearly empty interval
    u |= nfo["valid"] & (nfo["phi0"].abs() < FACE_MARGIN * h)                                 # face hit or march
    u |= hit & (which >= 0) & (which < 6) & X._close(nfo["t0"], nfo["second"], T_MARGIN)      # which face
    return u


def cast_field(cam, fields: Sequence, styles: Sequence, to_render, t: Tensor, shade: Tensor, hit: Tensor, hit_base: int = 0,
               dtype=torch.float64, margins: bool = False, step_factor: float = 1.0, max_steps: int = STEPS):
    """The field pass behind extras.collider_draw.cast: (t, shade, hit) - new tensors in `dtype` / int32 - with the field hits
    merged in [, unsure (H,W) bool, steps (H,W) int64: the march steps of the pixel's winning field hit, 0 elsewhere]."""
    H, W = int(cam.image_height), int(cam.image_width)
    N = H * W
    campos = X.ray_basis(cam)[1]
    o = X.sim_origin(campos, to_render).to(dtype)
    a = torch.tensor([float(v) for v in to_render[0]], dtype=dtype)
    dr = X.pixel_dirs(cam, dtype)
    ds = torch.stack([dr[:, k] / a[k] for k in range(3)], dim=-1)
    best_t = t.detach().cpu().to(dtype).reshape(N).clone()
    best = hit.detach().cpu().to(torch.int64).reshape(N).clone()
    rgb = shade.detach().cpu().to(dtype).reshape(3, N).clone()
    unsure = torch.zeros(N, dtype=torch.bool)
    steps = torch.zeros(N, dtype=torch.int64)
    for j, (c, st) in enumerate(zip(fields, styles)):
        if margins:
            is_hit, tf, which, n, nfo = trace(c, o, ds, best_t, True, step_factor, max_steps, info=True)
            unsure |= _unsure_rays(is_hit, tf, which, n, ds, nfo, max_steps)
            unsure |= is_hit & X._close(tf, best_t, T_MARGIN)                                 # a competing collider's t
        else:
            is_hit, tf, which, n = trace(c, o, ds, best_t, True, step_factor, max_steps)
        better = is_hit & (tf < best_t)
        nr = [n[:, k] / a[k] for k in range(3)]
        nl = torch.sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2])
        ndl = -(nr[0] * dr[:, 0] + nr[1] * dr[:, 1] + nr[2] * dr[:, 2]) / torch.where(nl > 0, nl, torch.ones_like(nl))
        ndl = torch.where(which < 0, torch.ones_like(ndl), ndl)
        lam = 0.35 + 0.65 * torch.clamp(ndl, min=0.0)
        for ch in range(3):
            rgb[ch] = torch.where(better, torch.tensor(float(st.color[ch]), dtype=dtype) * lam, rgb[ch])
        if margins:
            steps = torch.where(better, nfo["steps"], steps)
        best_t = torch.where(better, tf, best_t)
        best = torch.where(better, torch.full_like(best, hit_base + j), best)
    out = (best_t.reshape(H, W), rgb.reshape(3, H, W), best.to(torch.int32).reshape(H, W))
    if margins:
        return out + (unsure.reshape(H, W), steps.reshape(H, W))
    return out


def hidden_field(campos, fields: Sequence, means3D: Tensor, to_render=X.IDENTITY, hidden: Optional[Tensor] = None,
                 dtype=torch.float64, margins: bool = False):
    """(K,) bool: `hidden` (what the analytic colliders hide; none if None) or the Gaussian at means3D[i] (render coordinates) is
    hidden from campos by a field's drawn solid [, unsure (K,) bool]."""
    cam_r = torch.as_tensor(campos).detach().float().cpu().double().reshape(3)
    o = X.sim_origin(cam_r, to_render).to(dtype)
    a = torch.tensor([float(v) for v in to_render[0]], dtype=dtype)
    m = means3D.detach().cpu().to(dtype)
    cr = cam_r.to(dtype)
    ds = torch.stack([(m[:, k] - cr[k]) / a[k] for k in range(3)], dim=-1)
    K = m.shape[0]
    hid = torch.zeros(K, dtype=torch.bool) if hidden is None else hidden.detach().cpu().bool().clone()
    unsure = torch.zeros(K, dtype=torch.bool)
    ms = torch.stack([o[k] + ds[:, k] for k in range(3)], dim=-1)
    in_cube = ((ms >= 0) & (ms <= 1)).all(-1)
    cap = torch.ones(K, dtype=dtype)
    for c in fields:
        is_hit = trace(c, o, ds, cap, want_n=False)[0]
        inside, phi_m, _ = field_phi_normal(c, ms)
        hid |= is_hit | (in_cube & inside)
        if margins:
            is_hit, u, which, n, nfo = trace(c, o, ds, cap, want_n=True, info=True)
            unsure |= _unsure_rays(is_hit, u, which, n, ds, nfo)
            unsure |= is_hit & ((u - 1.0).abs() < SEGMENT_MARGIN)
            q = [(ms[:, k] - float(np.float32(c.origin[k]))) / float(np.float32(c.spacing)) for k in range(3)]
            on = in_cube & (q[0] >= 0) & (q[0] <= c.dims[0] - 1) & (q[1] >= 0) & (q[1] <= c.dims[1] - 1) & (q[2] >= 0) & (q[2] <= c.dims[2] - 1)
            unsure |= on & (phi_m.abs() < SEGMENT_MARGIN)
    return (hid, unsure) if margins else hid
