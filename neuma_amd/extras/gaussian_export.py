"""The 3DGS parametrisation of deformed Gaussians in numpy fp64: the CPU path of neuma_amd/export.py (as extras/gaussian_fill.py
is of gaussian_fill.py) and the yardstick its HIP kernel (csrc/nm_export.hip, nm_gaussian_deform) is held to.  The reference keeps
a deformed frame only as the six covariance numbers it hands its rasterizer and shows it in its own viewer; nothing in it writes one.

The factorisation, stated once for both paths:
    L      = build_rotation(normalize(rot)) diag(scale_modifier exp(log_scales))                        (`rest_factor`)
    M      = F L = U diag(s) V^T, U in SO(3) (a reflection goes into the sign of one s)                 (np.linalg.svd here)
    scales = max(|s_i|, floor), floor = max(1e-20 s_0, TINY); log_scales' = log(scales)
    rot'   = the unit quaternion of U with r >= 0, by Shepperd's branch on the largest of (trace, m00, m11, m22)   (`rot_to_quat`)
so that build_rotation(rot') diag(exp(log_scales'))^2 build_rotation(rot')^T = F L L^T F^T  (`covariance` of the outputs equals
`deformed_covariance` of the inputs).  F L L^T F^T itself is never decomposed: its eigenvalues are s^2, and a 100:1 Gaussian would
be known to half the digits.

TINY is the format's own "squares to zero": 1e-37 in the fp32 kernel, 1e-170 here, so a zero F activates to exactly the zero
covariance in either arithmetic while its log-scale stays finite (about -85 and -391)."""
from typing import Optional, Tuple

import numpy as np

REL_FLOOR = 1e-20
TINY = 1e-170


def build_rotation(q: np.ndarray) -> np.ndarray:
    """general_utils.py:101-124 for unit quaternions (K, 4) in (r, x, y, z) order -> (K, 3, 3)"""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), dtype=np.float64)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _f64(a, tail) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tail:
        raise ValueError(f"expected an array of shape (K, {', '.join(map(str, tail))}), got {a.shape}")
    return a


def rest_factor(log_scales, rot, scale_modifier: float = 1.0) -> np.ndarray:
    """L (K, 3, 3) with L L^T the covariance nm_gaussian_activate / build_cov3D give these raw parameters"""
    ls, q = _f64(log_scales, (3,)), _f64(rot, (4,))
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    return build_rotation(q) * (float(scale_modifier) * np.exp(ls))[:, None, :]


def covariance(log_scales, rot, scale_modifier: float = 1.0) -> np.ndarray:
    """the full (K, 3, 3) covariance of raw parameters"""
    Lm = rest_factor(log_scales, rot, scale_modifier)
    return Lm @ Lm.transpose(0, 2, 1)


def deformed_covariance(log_scales, rot, F=None, scale_modifier: float = 1.0) -> np.ndarray:
    """the definition: F L L^T F^T (K, 3, 3)"""
    M = rest_factor(log_scales, rot, scale_modifier)
    if F is not None:
        M = _f64(np.asarray(F).reshape(-1, 3, 3), (3, 3)) @ M
    return M @ M.transpose(0, 2, 1)


def strip_symmetric(S: np.ndarray) -> np.ndarray:
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=-1)


def rot_to_quat(R: np.ndarray) -> np.ndarray:
    """(K, 3, 3) rotations -> unit quaternions (K, 4), r >= 0.  Every branch is 4 c (r, x, y, z) with c the component that branch
    makes largest, so the factor leaves with the normalisation."""
    m = lambda i, j: R[:, i, j]
    t = m(0, 0) + m(1, 1) + m(2, 2)
    one = np.ones_like(t)
    cands = np.stack([
        np.stack([one + t, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
        np.stack([m(2, 1) - m(1, 2), one + m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)], -1),
        np.stack([m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), one - m(0, 0) + m(1, 1) - m(2, 2), m(1, 2) + m(2, 1)], -1),
        np.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), one - m(0, 0) - m(1, 1) + m(2, 2)], -1)], 1)
    pick = np.argmax(np.stack([t, m(0, 0), m(1, 1), m(2, 2)], -1), axis=1)          # (the first of equal ones: the trace)
    v = cands[np.arange(R.shape[0]), pick]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.where(v[:, :1] < 0, -v, v)


def gaussian_deform(log_scales, rot, F=None, scale_modifier: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """(log_scales' (K, 3), rot' (K, 4)) in fp64 of the Gaussians deformed by F (K, 3, 3) (None: the identity).  ValueError on bad
    shapes or non-finite input."""
    M = rest_factor(log_scales, rot, scale_modifier)
    if F is not None:
        Fm = _f64(np.asarray(F).reshape(-1, 3, 3), (3, 3))
        if Fm.shape[0] != M.shape[0]:
            raise ValueError(f"{Fm.shape[0]} deformation gradients for {M.shape[0]} Gaussians")
        M = Fm @ M
    if not np.isfinite(M).all():
        raise ValueError("non-finite Gaussian parameters or deformation gradients")
    U, s, _ = np.linalg.svd(M)
    U = U.copy()
    U[:, :, 2] *= np.where(np.linalg.det(U) < 0, -1.0, 1.0)[:, None]               # U in SO(3); s enters squared
    floor = np.maximum(REL_FLOOR * s[:, :1], TINY)
    return np.log(np.maximum(s, floor)), rot_to_quat(U)


def deformed_parameters(gaussians, means3D, deform_grad=None, shs=None, scaling_modifier: float = 1.0):
    """The CPU counterpart of export.deformed_gaussians: a new GaussianModel of CPU tensors (fp32, as the file stores them)."""
    import torch
    from ..render.gaussian_model import GaussianModel
    F = None if deform_grad is None else deform_grad.detach().cpu().numpy()
    ls, q = gaussian_deform(gaussians._scaling.detach().cpu().numpy(), gaussians._rotation.detach().cpu().numpy(), F, scaling_modifier)
    rest = gaussians._features_rest if shs is None else shs[:, 1:].contiguous()
    out = GaussianModel(gaussians.max_sh_degree)
    out.active_sh_degree = gaussians.active_sh_degree
    return out.set_params(means3D, gaussians._features_dc, rest, torch.from_numpy(ls.astype(np.float32)),
                          torch.from_numpy(q.astype(np.float32)), gaussians._opacity)
