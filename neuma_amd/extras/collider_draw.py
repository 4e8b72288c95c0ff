"""Drawing colliders in renders, as torch functions on the CPU: the DEFINITION the native kernels (csrc/nm_draw.hip,
csrc/nm_collide_ray.h) are held to, and the CPU path of neuma_amd.collider_draw.  The prose is in include/neuma_hip.h ("Drawing
colliders") and DESIGN.md section 7; in short

    drawn solid   shape cut by the unit cube [0,1]^3; a ray o + t d is inside for t in (t_in, t_out): largest entry, smallest exit
    pixel ray     from campos through the far-plane point that projmatrix maps to the pixel's centre
    hit           t_in < t_out and t_out > 0, at t = max(t_in, 0); the nearest over the colliders
    shade         color k (0.35 + 0.65 max(0, n_r.l)), l = -d_r; k = 0.8 on the odd cells of a plane's checkerboard
    hidden        the segment camera -> Gaussian mean meets a drawn solid before the mean, or the mean is inside one
    compose       rgb_front + (1 - a_front) shade where hit, img_all elsewhere

Everything is evaluated in `dtype`: fp64 is the yardstick; fp32 spells the kernels' operations in the kernels' order (they are
compiled without fma contraction), and its distance from fp64 is what the kernels' own distance is measured against.  With
`margins=True` the fp64 evaluation also returns which pixels / Gaussians sit so close to a branch (which constraint gives the
entry, hit or miss at a silhouette, which collider is nearest, the checker cell, hidden or shown) that fp32 may decide otherwise.

`colliders` is what neuma_amd.sim.colliders.parse_colliders returns, `styles` what neuma_amd.collider_draw.parse_styles returns
(objects with .color and .checker), `to_render` = (a, b) with p_render = a * p_sim + b per axis, `cam` anything with
image_height, image_width, full_proj_transform and camera_center (the row-vector convention of the rasterizer's cameras).
Not differentiated.  Nothing here imports the test oracle.
"""
import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ..sim.colliders import Box, Plane, Sphere

IDENTITY = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
ENTRY_MARGIN = 1e-4        # entry candidates, t_in / t_out, nearest two colliders: relative
CHECKER_MARGIN = 1e-3      # checker coordinate, in cells, from a cell border
SEGMENT_MARGIN = 1e-5      # |u_in - 1| of the segment test
_INF = float("inf")


def plane_frame(normal) -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
    """Deterministic 2-D frame (u, v) of a plane from its unit normal n, in fp64: e = the coordinate axis along which |n| is
    smallest (the lowest index of equal ones), u = normalize(n x e), v = n x u."""
    n = [float(a) for a in normal]
    e = 0
    if abs(n[1]) < abs(n[e]):
        e = 1
    if abs(n[2]) < abs(n[e]):
        e = 2
    ev = [1.0 if a == e else 0.0 for a in range(3)]
    u = [n[1] * ev[2] - n[2] * ev[1], n[2] * ev[0] - n[0] * ev[2], n[0] * ev[1] - n[1] * ev[0]]
    length = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    u = [a / length for a in u]
    v = [n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]]
    return tuple(u), tuple(v)


def inverse_projection(cam) -> Tensor:
    """projmatrix^-1 in fp64 (row-vector convention: hom = clip @ inverse)."""
    return torch.linalg.inv(cam.full_proj_transform.detach().double().cpu())


def ray_basis(cam) -> Tuple[Tensor, Tensor]:
    """(G (3,3) fp64, campos (3,) fp64): the direction of the ray through ndc (x, y) is x G[0] + y G[1] + G[2] times a positive
    number: hom.xyz - hom.w campos for hom = (x, y, 1, 1) @ projmatrix^-1, the far-plane point that projects to (x, y)."""
    inv = inverse_projection(cam)
    campos = cam.camera_center.detach().float().cpu().double().reshape(3)       # (the C ABI's nm_raster_cfg holds it in fp32)
    rows = torch.stack([inv[0], inv[1], inv[2] + inv[3]])
    return rows[:, :3] - rows[:, 3:4] * campos[None], campos


def sim_origin(campos: Tensor, to_render) -> Tensor:
    a, b = (torch.tensor([float(v) for v in t], dtype=torch.float64) for t in to_render)
    if not bool((a > 0).all()):
        raise ValueError(f"to_render: a <= 0 ({tuple(float(v) for v in a)})")
    return (campos - b.float().double()) / a.float().double()


def pixel_dirs(cam, dtype=torch.float64) -> Tensor:
    """Unit render-space directions (H*W, 3) of the pixel rays, row-major."""
    H, W = int(cam.image_height), int(cam.image_width)
    G = ray_basis(cam)[0].to(dtype)
    nx = (torch.arange(W) * 2 + 1).to(dtype) / torch.tensor(float(W), dtype=dtype) - 1.0
    ny = (torch.arange(H) * 2 + 1).to(dtype) / torch.tensor(float(H), dtype=dtype) - 1.0
    nx, ny = nx[None, :].expand(H, W).reshape(-1), ny[:, None].expand(H, W).reshape(-1)
    d = [nx * G[0, a] + ny * G[1, a] + G[2, a] for a in range(3)]
    length = torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return torch.stack([c / length for c in d], dim=-1)


def _slab(q, dq, lo, hi):
    """lo < q + t dq < hi -> (t0, t1); dq = 0: everything or nothing"""
    fwd, still = dq > 0, dq == 0
    inv = 1.0 / torch.where(still, torch.ones_like(dq), dq)
    a = (torch.where(fwd, lo, hi) - q) * inv
    b = (torch.where(fwd, hi, lo) - q) * inv
    inside = ((q > lo) & (q < hi)).expand_as(dq)
    pinf, ninf = torch.full_like(dq, _INF), torch.full_like(dq, -_INF)
    return torch.where(still, torch.where(inside, ninf, pinf), a), torch.where(still, torch.where(inside, pinf, ninf), b)


def ray_solid(c, o: Tensor, d: Tensor):
    """One collider's drawn solid against the rays o + t d (o (3,), d (N,3), one dtype): t_in, t_out (N,), which (N,) int64 (the
    constraint of the entry: 0..2 the shape, 3..5 the cube's axis), n (N,3) the outward normal there in simulation coordinates
    (not normalised) and t_in2, the largest entry among the OTHER constraints (-inf if none)."""
    dt, N = d.dtype, d.shape[0]

    def s(v):
        return torch.tensor(float(v), dtype=dt)

    centre = c.point if isinstance(c, Plane) else c.center
    m = [o[a] - s(centre[a]) for a in range(3)]
    dd = [d[:, a] for a in range(3)]
    pinf, ninf = torch.full((N,), _INF, dtype=dt), torch.full((N,), -_INF, dtype=dt)
    which = torch.zeros(N, dtype=torch.int64)
    t_in2 = ninf.clone()
    if isinstance(c, Plane):
        nn = [s(v) for v in c.normal]
        s0 = nn[0] * m[0] + nn[1] * m[1] + nn[2] * m[2]
        sd = nn[0] * dd[0] + nn[1] * dd[1] + nn[2] * dd[2]
        tt = -s0 / torch.where(sd == 0, torch.ones_like(sd), sd)
        inside = (s0 < 0).expand(N)
        t_in = torch.where(sd < 0, tt, torch.where((sd > 0) | inside, ninf, pinf))
        t_out = torch.where(sd > 0, tt, torch.where((sd < 0) | inside, pinf, ninf))
        n = torch.stack([v.expand(N) for v in nn], dim=-1)
    elif isinstance(c, Sphere):
        A = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]
        bA = (m[0] * dd[0] + m[1] * dd[1] + m[2] * dd[2]) / A
        q = [m[a] - bA * dd[a] for a in range(3)]
        r = s(c.radius)
        e = r * r - (q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        h0 = torch.sqrt(e.abs() / A)
        h = torch.where(e > 0, h0, -h0)        # a line that misses the sphere gets the mirrored (empty) interval
        t_in, t_out = -bA - h, -bA + h
        n = torch.stack([m[a] + t_in * dd[a] for a in range(3)], dim=-1)
    elif isinstance(c, Box):
        R = [s(v) for v in c.rot]
        t_in, t_out, n = ninf.clone(), pinf.clone(), torch.zeros(N, 3, dtype=dt)
        for a in range(3):
            q = R[a] * m[0] + R[3 + a] * m[1] + R[6 + a] * m[2]
            dq = R[a] * dd[0] + R[3 + a] * dd[1] + R[6 + a] * dd[2]
            t0, t1 = _slab(q, dq, -s(c.half[a]), s(c.half[a]))
            better = t0 > t_in
            t_in2 = torch.where(better, t_in, torch.maximum(t_in2, t0))
            t_in = torch.where(better, t0, t_in)
            which = torch.where(better, torch.full_like(which, a), which)
            sg = torch.where(dq > 0, -torch.ones_like(dq), torch.ones_like(dq))
            n = torch.where(better[:, None], torch.stack([sg * R[a], sg * R[3 + a], sg * R[6 + a]], dim=-1), n)
            t_out = torch.minimum(t_out, t1)
    else:
        raise TypeError(f"not a collider: {c!r}")
    zero, one = s(0.0), s(1.0)
    for a in range(3):
        t0, t1 = _slab(o[a], dd[a], zero, one)
        better = t0 > t_in
        t_in2 = torch.where(better, t_in, torch.maximum(t_in2, t0))
        t_in = torch.where(better, t0, t_in)
        which = torch.where(better, torch.full_like(which, 3 + a), which)
        sg = torch.where(dd[a] > 0, -torch.ones_like(dd[a]), torch.ones_like(dd[a]))
        face = torch.zeros(N, 3, dtype=dt)
        face[:, a] = sg
        n = torch.where(better[:, None], face, n)
        t_out = torch.minimum(t_out, t1)
    return t_in, t_out, which, n, t_in2


def _close(x: Tensor, y: Tensor, rel: float) -> Tensor:
    """|x - y| < rel max(|x|, |y|), false where either is infinite"""
    fin = torch.isfinite(x) & torch.isfinite(y)
    return fin & ((x - y).abs() < rel * torch.maximum(x.abs(), y.abs()))


def cast(cam, colliders: Sequence, styles: Sequence, to_render=IDENTITY, dtype=torch.float64, margins: bool = False):
    """t (H,W; +inf where nothing is hit), shade (3,H,W), hit (H,W int32: collider index or -1) [, unsure (H,W) bool]."""
    H, W = int(cam.image_height), int(cam.image_width)
    N = H * W
    campos = ray_basis(cam)[1]
    o = sim_origin(campos, to_render).to(dtype)
    a = torch.tensor([float(v) for v in to_render[0]], dtype=dtype)
    dr = pixel_dirs(cam, dtype)
    ds = torch.stack([dr[:, k] / a[k] for k in range(3)], dim=-1)
    best_t = torch.full((N,), _INF, dtype=dtype)
    best_t2 = best_t.clone()
    best = torch.full((N,), -1, dtype=torch.int64)
    rgb = torch.zeros(3, N, dtype=dtype)
    unsure = torch.zeros(N, dtype=torch.bool)
    border = torch.zeros(N, dtype=torch.bool)
    for i, (c, st) in enumerate(zip(colliders, styles)):
        t_in, t_out, which, n, t_in2 = ray_solid(c, o, ds)
        is_hit = (t_in < t_out) & (t_out > 0)
        t = torch.clamp(t_in, min=0.0)
        better = is_hit & (t < best_t)
        nr = [n[:, k] / a[k] for k in range(3)]
        nl = torch.sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2])
        ndl = -(nr[0] * dr[:, 0] + nr[1] * dr[:, 1] + nr[2] * dr[:, 2]) / nl
        ndl = torch.where(t_in < 0, torch.ones_like(ndl), ndl)
        k = torch.ones(N, dtype=dtype)
        near_border = torch.zeros(N, dtype=torch.bool)
        if isinstance(c, Plane) and float(st.checker) > 0.0:
            u, v = plane_frame(c.normal)
            size = torch.tensor(float(st.checker), dtype=dtype)
            r = [o[j] + t * ds[:, j] - torch.tensor(float(c.point[j]), dtype=dtype) for j in range(3)]
            u, v = ([torch.tensor(float(x), dtype=dtype) for x in w] for w in (u, v))
            cu = (r[0] * u[0] + r[1] * u[1] + r[2] * u[2]) / size
            cv = (r[0] * v[0] + r[1] * v[1] + r[2] * v[2]) / size
            on_face = (which == 0) & ~(t_in < 0)
            fin = torch.isfinite(cu) & torch.isfinite(cv)
            cells = torch.where(fin, torch.floor(cu), torch.zeros_like(cu)).long() + torch.where(fin, torch.floor(cv), torch.zeros_like(cv)).long()
            k = torch.where(on_face & (cells % 2 == 1), torch.full_like(k, 0.8), k)
            near_border = on_face & fin & (((cu - torch.round(cu)).abs() < CHECKER_MARGIN) | ((cv - torch.round(cv)).abs() < CHECKER_MARGIN))
        lam = 0.35 + 0.65 * torch.clamp(ndl, min=0.0)
        col = [torch.tensor(float(x), dtype=dtype) for x in st.color]
        for ch in range(3):
            rgb[ch] = torch.where(better, col[ch] * k * lam, rgb[ch])
        if margins:
            unsure |= _close(t_in, t_out, ENTRY_MARGIN)                                     # silhouette: hit or miss
            unsure |= is_hit & (t_in > 0) & _close(t_in, t_in2, ENTRY_MARGIN)               # which constraint gives the entry
            border = torch.where(better, near_border, border)
            # the nearest two colliders: best_t2 = the second smallest t so far
            tt = torch.where(is_hit, t, torch.full_like(t, _INF))
            best_t2 = torch.where(better, best_t, torch.minimum(best_t2, tt))
        best_t = torch.where(better, t, best_t)
        best = torch.where(better, torch.full_like(best, i), best)
    out = (best_t.reshape(H, W), rgb.reshape(3, H, W), best.to(torch.int32).reshape(H, W))
    if margins:
        # (two solids entered through the same cube face give the same t, bit for bit, in any precision: the first in list
        # order wins, and that is no rounding-sensitive decision)
        unsure |= border | (_close(best_t, best_t2, ENTRY_MARGIN) & (best_t != best_t2))
        return out + (unsure.reshape(H, W),)
    return out


def hidden(campos, colliders: Sequence, means3D: Tensor, to_render=IDENTITY, dtype=torch.float64, margins: bool = False):
    """(K,) bool: is the Gaussian at means3D[i] (render coordinates) hidden from campos (render coordinates)? [, unsure (K,) bool]"""
    cam_r = torch.as_tensor(campos).detach().float().cpu().double().reshape(3)
    o = sim_origin(cam_r, to_render).to(dtype)
    a = torch.tensor([float(v) for v in to_render[0]], dtype=dtype)
    m = means3D.detach().cpu().to(dtype)
    cr = cam_r.to(dtype)
    ds = torch.stack([(m[:, k] - cr[k]) / a[k] for k in range(3)], dim=-1)
    hid = torch.zeros(m.shape[0], dtype=torch.bool)
    unsure = torch.zeros_like(hid)
    for c in colliders:
        u_in, u_out, _, _, _ = ray_solid(c, o, ds)
        hid |= (u_in < u_out) & (u_out > 0) & (u_in < 1)
        if margins:
            unsure |= _close(u_in, u_out, ENTRY_MARGIN) | ((u_in - 1.0).abs() < SEGMENT_MARGIN)
    return (hid, unsure) if margins else hid


def compose(img_all: Tensor, rgb_front: Tensor, a_front: Tensor, shade: Tensor, hit: Tensor, rows: Optional[Tuple[int, int]] = None,
            out: Optional[Tensor] = None) -> Tensor:
    """out (3,H,W) = rgb_front + (1 - a_front) shade where hit >= 0, img_all elsewhere; a_front (H,W).  rows = (y0, y1): only
    those pixel rows are written (into `out`, or into zeros)."""
    full = torch.where((hit >= 0)[None], rgb_front + (1.0 - a_front)[None] * shade, img_all)
    if rows is None:
        return full
    res = torch.zeros_like(img_all) if out is None else out.clone()
    res[:, rows[0]:rows[1]] = full[:, rows[0]:rows[1]]
    return res
