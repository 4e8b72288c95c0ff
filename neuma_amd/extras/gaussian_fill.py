"""Particles out of the Gaussians' own density field, in numpy fp64: the CPU path of neuma_amd/gaussian_fill.py (as
extras/mesh_sampling.py is of mesh_inside.py) and the yardstick its HIP kernels (csrc/nm_fill.hip) are held to.  Nothing in the
reference does this: it sends its users to outside meshing tools and a prebuilt sampler for particles.ply.

The algorithm, stated once for both paths:
    lattice    r = sqrt(cutoff diag(Sigma)), lo = min_k(mu - r), hi = max_k(mu + r), h = max(hi - lo) / resolution,
               dims = max(ceil((hi - lo) / h), 1); linear cell index (ix ny + iy) nz + iz              (`fill_lattice`)
    density    at the cell centre c = lo + (i + 1/2) h:  d(c) = sum_k [m_k <= cutoff] o_k exp(-m_k / 2),
               m_k = (c - mu_k)^T inv(Sigma_k) (c - mu_k), the inverse by cofactors, the terms added in ascending k.  A Gaussian
               whose covariance has a non-positive or non-finite determinant contributes nothing       (`density_field`)
    classify   shell = d > density_thres; enclosed = not shell, and on each of the three axis lines through the cell a shell
               cell at a strictly lower and one at a strictly higher index (six rays)                  (`classify_cells`)
    emit       enclosed cells, plus the shell ones when include_shell, in ascending linear index; per cell per_cell^3 points
               lo_a + (i_a + (s_a + 1/2) / per_cell) h with s nested x, y, z, each coordinate evaluated in fp64 by that one
               expression and rounded to fp32 once                                                      (`emit_points`)
Both paths evaluate a Gaussian only at the cells of the 4 x 4 x 4 blocks under the box of its cutoff ellipsoid
(`gaussian_blocks`); the box holds the whole ellipsoid, so that changes no value.

`density_thres` = 0.5 is a default nobody has tuned on a real capture yet."""
from typing import Dict, Tuple

import numpy as np

BLOCK = 4                    # cells per block edge of the native path (csrc/nm_fill.hip)
MAX_CELLS = 1 << 27
_INT32_MAX = np.iinfo(np.int32).max


def _inputs(means, cov6, opacity=None):
    """(means (K, 3), cov6 (K, 6)[, opacity (K,)]) as the fp32 arrays both paths start from, or ValueError (K = 0, bad
    shapes, a non-finite value)."""
    mu = np.ascontiguousarray(np.asarray(means, dtype=np.float32))
    cv = np.ascontiguousarray(np.asarray(cov6, dtype=np.float32))
    if mu.ndim != 2 or mu.shape[1] != 3 or cv.ndim != 2 or cv.shape[1] != 6 or len(cv) != len(mu):
        raise ValueError(f"means must be (K, 3) and cov6 (K, 6), got {mu.shape} and {cv.shape}")
    if len(mu) == 0:
        raise ValueError("no Gaussians to fill (K = 0)")
    if not (np.isfinite(mu).all() and np.isfinite(cv).all()):
        raise ValueError("means / cov6 hold non-finite values")
    if opacity is None:
        return mu, cv
    op = np.ascontiguousarray(np.asarray(opacity, dtype=np.float32).reshape(-1))
    if len(op) != len(mu):
        raise ValueError(f"opacity must be (K,), got {op.shape} for K = {len(mu)}")
    if not np.isfinite(op).all():
        raise ValueError("opacity holds non-finite values")
    return mu, cv, op


def _cutoff(cutoff) -> float:
    c = float(np.float32(cutoff))         # the native path takes it as fp32
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"cutoff must be positive and finite, got {cutoff}")
    return c


def gaussian_blocks(means, cov6, origin, h, dims, cutoff=9.0) -> Tuple[np.ndarray, np.ndarray]:
    """(b0, b1) (K, 3) int64: lowest and highest 4^3 block per axis under the box of each Gaussian's cutoff ellipsoid (half
    extent sqrt(cutoff Sigma_ii), inflated by 1e-4 against the fp32 rounding of m), clamped to the lattice.  fp64, the same
    expressions as k_fill_gaussians."""
    mu, cv = _inputs(means, cov6)
    mu, diag = mu.astype(np.float64), cv[:, [0, 3, 5]].astype(np.float64)
    e = np.sqrt(np.maximum(_cutoff(cutoff) * diag, 0.0)) * 1.0001 + 1e-12
    top = np.asarray(dims, dtype=np.float64) - 1.0
    c0 = np.clip(np.floor((mu - e - origin) / h), 0.0, top).astype(np.int64)
    c1 = np.clip(np.floor((mu + e - origin) / h), 0.0, top).astype(np.int64)
    return c0 // BLOCK, c1 // BLOCK


def fill_lattice(means, cov6, resolution: int, cutoff=9.0) -> Tuple[np.ndarray, float, np.ndarray]:
    """(origin (3,) fp64, h, dims (3,) int64) of the lattice both paths fill, from the fp32 inputs in fp64.  ValueError: K = 0,
    non-finite inputs, resolution < 1, no extent, more than 2^27 cells, or more (Gaussian, block) pairs than an int32 holds."""
    mu, cv = _inputs(means, cov6)
    if int(resolution) < 1 or int(resolution) != resolution:
        raise ValueError(f"resolution must be an integer >= 1, got {resolution}")
    mu, diag = mu.astype(np.float64), cv[:, [0, 3, 5]].astype(np.float64)
    r = np.sqrt(np.maximum(_cutoff(cutoff) * diag, 0.0))
    lo, hi = (mu - r).min(0), (mu + r).max(0)
    h = float((hi - lo).max()) / int(resolution)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("the Gaussians span no volume (all covariances zero and all centres equal?)")
    fd = np.maximum(np.ceil((hi - lo) / h), 1.0)
    if float(fd.prod()) > MAX_CELLS:
        raise ValueError(f"lattice of {int(fd[0])} x {int(fd[1])} x {int(fd[2])} cells is larger than 2^27: lower `resolution`")
    dims = fd.astype(np.int64)
    b0, b1 = gaussian_blocks(means, cov6, lo, h, dims, cutoff)
    pairs = int((b1 - b0 + 1).prod(1).sum())
    if pairs > _INT32_MAX:
        raise ValueError(f"{pairs} (Gaussian, block) pairs do not fit an int32: lower `resolution` or prune large Gaussians")
    return lo, h, dims


def inverse_cov(cov6, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """(A (K, 6), ok (K,)): the six unique entries of inv(Sigma) by cofactors, evaluated in `dtype`, and which Gaussians count.
    `ok` is decided in fp64 whatever `dtype` is, exactly as k_fill_gaussians decides it: the determinant is a positive finite
    number and the fp64 inverse fits fp32."""
    def cof(s):
        s00, s01, s02, s11, s12, s22 = (s[:, i] for i in range(6))
        c = (s11 * s22 - s12 * s12, s12 * s02 - s01 * s22, s01 * s12 - s11 * s02,
             s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01)
        return c, s00 * c[0] + s01 * c[1] + s02 * c[2]

    s = np.asarray(cov6, dtype=np.float32)
    with np.errstate(all="ignore"):
        c64, det64 = cof(s.astype(np.float64))
        a64 = np.stack([c / det64 for c in c64], 1)
        ok = (det64 > 0) & np.isfinite(det64) & np.isfinite(a64.astype(np.float32)).all(1)
        if np.dtype(dtype) == np.float64:
            a = a64
        else:
            c, det = cof(s.astype(dtype))
            a = np.stack([x / det for x in c], 1)
    return np.where(ok[:, None], a, 0).astype(dtype), ok


def density_field(means, cov6, opacity, origin, h, dims, cutoff=9.0, dtype=np.float64) -> Tuple[np.ndarray, int]:
    """(field (ncells,) `dtype`, number of Gaussians skipped as degenerate).  `dtype` = fp64 is the yardstick; fp32 evaluates
    inv(Sigma), c - mu, m, exp and the sum in fp32 from the same fp32-rounded cell centres, which is what fp32 evaluation
    alone costs against it."""
    mu, cv, op = _inputs(means, cov6, opacity)
    dt = np.dtype(dtype).type
    cut = dt(_cutoff(cutoff))
    dims = np.asarray(dims, dtype=np.int64)
    origin = np.asarray(origin, dtype=np.float64)
    A, ok = inverse_cov(cv, dtype)
    b0, b1 = gaussian_blocks(mu, cv, origin, h, dims, cutoff)
    # cell centres per axis: fp64, rounded to fp32 once (the native path's), then taken to `dtype`
    cen = [(origin[a] + (np.arange(dims[a], dtype=np.float64) + 0.5) * h).astype(np.float32).astype(dtype) for a in range(3)]
    field = np.zeros(tuple(dims), dtype=dtype)
    mu, op = mu.astype(dtype), op.astype(dtype)
    two, half = dt(2), dt(0.5)
    for k in np.flatnonzero(ok):
        sl = tuple(slice(int(b0[k, a]) * BLOCK, min((int(b1[k, a]) + 1) * BLOCK, int(dims[a]))) for a in range(3))
        dx = (cen[0][sl[0]] - mu[k, 0])[:, None, None]
        dy = (cen[1][sl[1]] - mu[k, 1])[None, :, None]
        dz = (cen[2][sl[2]] - mu[k, 2])[None, None, :]
        a = A[k]
        m = dx * (a[0] * dx + two * (a[1] * dy + a[2] * dz)) + dy * (a[3] * dy + two * (a[4] * dz)) + a[5] * dz * dz
        field[sl] += np.where(m <= cut, op[k] * np.exp(-half * m), dt(0))
    return field.reshape(-1), int((~ok).sum())


def classify_cells(field, dims, density_thres=0.5) -> np.ndarray:
    """kind (ncells,) uint8 of any field: 1 = shell (field > density_thres, compared in the field's own precision), 2 =
    enclosed (not shell, shell cells strictly below and strictly above it on all three axis lines), 0 = outside."""
    f = np.asarray(field)
    dims = tuple(int(d) for d in dims)
    if f.size != dims[0] * dims[1] * dims[2]:
        raise ValueError(f"field of {f.size} cells does not match dims {dims}")
    f = f.reshape(dims)
    shell = f > f.dtype.type(density_thres)
    enclosed = ~shell
    for ax in range(3):
        n = dims[ax]
        idx = np.arange(n).reshape([n if a == ax else 1 for a in range(3)])
        first = np.where(shell, idx, n).min(ax, keepdims=True)
        last = np.where(shell, idx, -1).max(ax, keepdims=True)
        enclosed &= (first < idx) & (idx < last)
    return (shell.astype(np.uint8) + 2 * enclosed.astype(np.uint8)).reshape(-1)


def emit_points(kind_cell, origin, h, dims, per_cell: int = 1, include_shell: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """(points (M, 3) fp32, kind (M,) uint8) of the kept cells in ascending linear index, per_cell^3 points each."""
    n = int(per_cell)
    if n < 1:
        raise ValueError(f"per_cell must be >= 1, got {per_cell}")
    kc = np.asarray(kind_cell, dtype=np.uint8).reshape(-1)
    dims = np.asarray(dims, dtype=np.int64)
    origin = np.asarray(origin, dtype=np.float64)
    cells = np.flatnonzero((kc == 2) | ((kc == 1) & bool(include_shell)))
    idx = np.stack(np.unravel_index(cells, tuple(dims)), 1).astype(np.float64).reshape(-1, 3)       # (M, 3) cell coordinates
    s = np.stack(np.meshgrid(*([np.arange(n, dtype=np.float64)] * 3), indexing="ij"), -1).reshape(-1, 3)      # x, y, z nested
    pts = origin[None, None, :] + (idx[:, None, :] + (s[None, :, :] + 0.5) / float(n)) * float(h)
    return pts.reshape(-1, 3).astype(np.float32), np.repeat(kc[cells], n ** 3)


def fill_from_gaussians(means, cov6, opacity, resolution: int = 64, density_thres: float = 0.5, cutoff: float = 9.0,
                        per_cell: int = 1, include_shell: bool = True) -> Tuple[np.ndarray, np.ndarray, Dict]:
    """(points (M, 3) fp32, kind (M,) uint8: 1 shell / 2 enclosed, info) - the whole fill on the CPU.  info: dims, h, origin,
    n_shell, n_enclosed (cells of each kind, emitted or not), n_skipped (degenerate Gaussians).  `density_thres` = 0.5 has
    not been chosen on a real capture.  Nothing to emit is a (0, 3) array, not an error."""
    if int(per_cell) < 1:
        raise ValueError(f"per_cell must be >= 1, got {per_cell}")
    mu, cv, op = _inputs(means, cov6, opacity)
    origin, h, dims = fill_lattice(mu, cv, resolution, cutoff)
    field, skipped = density_field(mu, cv, op, origin, h, dims, cutoff)
    kc = classify_cells(field, dims, density_thres)
    points, kind = emit_points(kc, origin, h, dims, per_cell, include_shell)
    info = dict(dims=tuple(int(d) for d in dims), h=h, origin=origin, n_shell=int((kc == 1).sum()), n_enclosed=int((kc == 2).sum()),
                n_skipped=skipped)
    return points, kind, info
