"""Rigid edits of a Gaussian set, the counterpart of the reference's modules/d3gs/utils/transform_utils.py:
translate_gaussians, scale_gaussians, rotate_gaussians, rotate_transform, quaternion_multiply and the rotation of the SH
colour coefficients (transform_shs_by_rotmat / transform_shs_by_quat).

SH rotation.  For a rotation R (as in `points @ R.T`) and coefficients c (K, M, 3) the rotated coefficients are
c' = diag(1, D_1, D_2, D_3) c per Gaussian and colour channel, with D defined by  sum_j c'_j Y_j(R d) = sum_j c_j Y_j(d)
for every unit d: moving the Gaussians and the camera by the same rigid motion leaves the image unchanged.  Y_j is the
rasterizer's real basis (k_preprocess of nm_raster.hip; the constants below).  Because D is orthogonal the definition is
Y_l(R d) = D_l Y_l(d), and every Y_l is a homogeneous polynomial of degree l in d, so with 2l+1 fixed directions s_k

    D_l(R) = [Y_l(R s_1) ... Y_l(R s_{2l+1})]  A_l^{-1},      A_l = [Y_l(s_1) ... Y_l(s_{2l+1})]   (a constant),

a polynomial of degree l in the nine entries of R: no angles, no singular pose.  `sh_rotation_matrices` is that formula
in torch (differentiable, any dtype / device); nm_shrot.hip evaluates the same formula with the same directions and the
same A_l^{-1} (tools/gen_shrot_tables.py writes its table from `sh_rotation_tables`).  The reference reaches D through
e3nn's wigner_D and Euler angles; e3nn is not a dependency here and parity with its numbers is unpinned."""
from functools import lru_cache
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L

# the rasterizer's SH constants (nm_raster.hip k_preprocess; sh_utils.py:26-51 of the reference)
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)

# Sample directions (normalised in fp64); band l uses the first 2l+1.  Picked from small-integer vectors for the
# conditioning of A_l: cond(A_1) = 1.8, cond(A_2) = 3.2, cond(A_3) = 3.2.
SH_ROT_DIRS = ((-2, -2, 0), (0, -3, 3), (-3, 2, 2), (3, 0, 0), (2, -2, 1), (-1, -2, -3), (-3, -3, -2))

_REST_ROWS = {3: 1, 8: 2, 15: 3}       # rows of a _features_rest -> its SH degree


def sh_band(l: int, p):
    """Y_l at the points p (..., 3) as homogeneous polynomials (no normalisation of p): (..., 2l+1), in the rasterizer's
    coefficient order.  Works on torch tensors and numpy arrays."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    stack = torch.stack if isinstance(p, Tensor) else np.stack
    if l == 1:
        return stack([-SH_C1 * y, SH_C1 * z, -SH_C1 * x], -1)
    xx, yy, zz = x * x, y * y, z * z
    if l == 2:
        return stack([SH_C2[0] * (x * y), SH_C2[1] * (y * z), SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * (x * z),
                      SH_C2[4] * (xx - yy)], -1)
    if l == 3:
        return stack([SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * (x * y) * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
                      SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy),
                      SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3.0 * yy)], -1)
    raise ValueError(f"sh_band: band {l} (1..3)")


@lru_cache(maxsize=None)
def sh_rotation_tables():
    """(dirs (7,3) fp64 unit rows, (A_1^{-1}, A_2^{-1}, A_3^{-1}) fp64) as numpy arrays: the constants of the formula."""
    d = np.asarray(SH_ROT_DIRS, dtype=np.float64)
    d = d / np.sqrt((d * d).sum(1, keepdims=True))
    ainv = tuple(np.linalg.inv(sh_band(l, d[:2 * l + 1]).T) for l in (1, 2, 3))      # A_l[i][k] = Y_i(s_k)
    return d, ainv


def sh_rotation_matrices(R: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(D_1 (3,3), D_2 (5,5), D_3 (7,7)) of the rotation matrix R (3,3); differentiable in R."""
    assert R.shape == (3, 3), f"Rotation matrix must have shape (3, 3), but got {R.shape}."
    dirs, ainv = sh_rotation_tables()
    out = []
    for l in (1, 2, 3):
        s = torch.as_tensor(dirs[:2 * l + 1], dtype=R.dtype, device=R.device)
        yr = sh_band(l, s @ R.T)                                   # [k][i] = Y_i(R s_k)
        out.append(yr.T @ torch.as_tensor(ainv[l - 1], dtype=R.dtype, device=R.device))
    return tuple(out)


def _rest_degree(shs_feat: Tensor) -> int:
    assert shs_feat.dim() == 3 and shs_feat.shape[-1] == 3, f"SH features must be in RGB format (N, SHS_NUM, 3), but got {tuple(shs_feat.shape)}"
    rows = shs_feat.shape[1]
    if rows not in _REST_ROWS:
        raise ValueError(f"SH features without the DC row must have 3, 8 or 15 rows (sh_degree 1, 2, 3), but got {rows}")
    return _REST_ROWS[rows]


def rotate_shs_torch(shs_feat: Tensor, R: Tensor) -> Tensor:
    """transform_shs_by_rotmat through torch ops (`sh_rotation_matrices` + one einsum per band): the differentiable path
    of Register.forward and the tests' yardstick.  shs_feat (K, 3 | 8 | 15, 3) -> a new tensor."""
    if shs_feat.shape[1] <= 1:
        return shs_feat
    deg = _rest_degree(shs_feat)
    D = sh_rotation_matrices(R.to(shs_feat.dtype))
    parts, lo = [], 0
    for l in range(1, deg + 1):
        parts.append(torch.einsum("ij,kjc->kic", D[l - 1], shs_feat[:, lo:lo + 2 * l + 1]))
        lo += 2 * l + 1
    return torch.cat(parts, 1)


def rotate_shs_per_gaussian_torch(shs_rest: Tensor, R: Tensor) -> Tensor:
    """One rotation per Gaussian through torch ops: shs_rest (K, 3 | 8 | 15, 3), R (K, 3, 3) -> a new tensor, any dtype and
    device.  The D_l are not formed: with w = A_l^{-1} c_l per channel, c'_l,i = sum_k Y_l,i(R s_k) w_k - the formula of
    nm_sh_rotate_polar, its CPU path and the tests' yardstick, as `rotate_shs_torch` is for one R."""
    if shs_rest.shape[1] <= 1:
        return shs_rest
    deg = _rest_degree(shs_rest)
    assert R.shape == (shs_rest.shape[0], 3, 3), f"Rotations must have shape ({shs_rest.shape[0]}, 3, 3), but got {tuple(R.shape)}."
    R = R.to(shs_rest)
    dirs, ainv = sh_rotation_tables()
    parts, lo = [], 0
    for l in range(1, deg + 1):
        n = 2 * l + 1
        s = torch.as_tensor(dirs[:n], dtype=R.dtype, device=R.device)
        yv = sh_band(l, torch.einsum("gab,kb->gka", R, s))                                # [g][k][i] = Y_i(R_g s_k)
        w = torch.einsum("kj,gjc->gkc", torch.as_tensor(ainv[l - 1], dtype=R.dtype, device=R.device), shs_rest[:, lo:lo + n])
        parts.append(torch.einsum("gki,gkc->gic", yv, w))
        lo += n
    return torch.cat(parts, 1)


def rotate_shs_by_deformation(shs: Tensor, F: Tensor, has_dc: bool = True, return_rotation: bool = False):
    """nm_sh_rotate_polar: the colours of a roll-out frame turned with each Gaussian's own deformation.  shs (K, n, 3) and the
    bound deformation gradients F (K, 3, 3), both GPU fp32; R_g = U Vh of the project's SVD of F_g (the rotation of the polar
    decomposition) and c'_g = diag(1, D_1(R_g), D_2(R_g), D_3(R_g)) c_g.  Returns a NEW tensor, or (it, R (K, 3, 3)) with
    `return_rotation`; `shs` with one row or fewer is returned as is (R is then None).  Not differentiable: the colour's
    dependence on F is not propagated, so inputs that require grad are refused while grad mode is on.  The reference has no
    counterpart (its shs reach the rasterizer unrotated)."""
    assert shs.dim() == 3 and shs.shape[-1] == 3, f"SH features must be in RGB format (N, SHS_NUM, 3), but got {tuple(shs.shape)}"
    if torch.is_grad_enabled() and (shs.requires_grad or F.requires_grad):
        raise RuntimeError("rotate_shs_by_deformation is not differentiable: the colour's dependence on F is not propagated "
                           "(call it under torch.no_grad() or on detached tensors)")
    if shs.shape[1] <= 1:
        return (shs, None) if return_rotation else shs
    Fc = F.detach().reshape(-1, 3, 3).contiguous()
    sc = shs.detach().contiguous()
    assert Fc.shape[0] == sc.shape[0], f"Shape mismatch: shs {sc.shape[0]} F {Fc.shape[0]}"
    dev = L.same_device(sc, Fc)
    out = torch.empty_like(sc)
    R = torch.empty_like(Fc) if return_rotation else None
    L.check(L.lib().nm_sh_rotate_polar(sc.shape[0], sc.shape[1], int(has_dc), L.ptr(Fc, torch.float32), L.ptr(sc, torch.float32),
                                       L.ptr(out, torch.float32), L.ptr(R), L.stream_ptr(dev)), "nm_sh_rotate_polar")
    return (out, R) if return_rotation else out


def sh_rotate(shs: Tensor, R9: Tensor, has_dc: bool, out: Optional[Tensor] = None) -> Tensor:
    """nm_sh_rotate: shs (K, n, 3) fp32 on the GPU, R9 nine DEVICE floats (row-major); `out` may be `shs` itself."""
    out = torch.empty_like(shs) if out is None else out
    L.check(L.lib().nm_sh_rotate(shs.shape[0], shs.shape[1], int(has_dc), L.ptr(R9, torch.float32), L.ptr(shs, torch.float32),
                                 L.ptr(out, torch.float32), L.stream_ptr(L.same_device(shs, R9, out))), "nm_sh_rotate")
    return out


def sh_rotate_backward(shs: Tensor, R9: Tensor, has_dc: bool, grad_out: Tensor, dR9: Tensor, want_dshs: bool = True,
                       workspace: Optional[Tensor] = None) -> Optional[Tensor]:
    """nm_sh_rotate_backward: dR9 (9 device floats) += the adjoint reduced over the Gaussians; returns dL/dshs (or None)."""
    lib = L.lib()
    k = shs.shape[0]
    nbytes = int(lib.nm_sh_rotate_bwd_workspace(k))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=shs.device)
    dshs = torch.empty_like(shs) if want_dshs else None
    L.check(lib.nm_sh_rotate_backward(k, shs.shape[1], int(has_dc), L.ptr(R9, torch.float32), L.ptr(shs, torch.float32),
                                      L.ptr(grad_out, torch.float32), L.ptr(dR9, torch.float32), L.ptr(dshs), L.ptr(workspace),
                                      workspace.numel(), L.stream_ptr(L.same_device(shs, R9, grad_out, dR9))), "nm_sh_rotate_backward")
    return dshs


class _ShRotate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shs_feat, R):
        shs = shs_feat.detach().contiguous()
        R9 = R.detach().reshape(9).contiguous()
        ctx.save_for_backward(shs, R9)
        return sh_rotate(shs, R9, False)

    @staticmethod
    def backward(ctx, grad_out):
        shs, R9 = ctx.saved_tensors
        dR9 = torch.zeros(9, dtype=torch.float32, device=shs.device)
        dshs = sh_rotate_backward(shs, R9, False, grad_out.contiguous(), dR9, want_dshs=ctx.needs_input_grad[0])
        return dshs, (dR9.reshape(3, 3) if ctx.needs_input_grad[1] else None)


def transform_shs_by_rotmat(shs_feat: Tensor, rotation_matrix: Tensor) -> Tensor:
    """transform_utils.py:41-104 on the native kernels: shs_feat (K, 3 | 8 | 15, 3) (a `_features_rest`, no DC row) rotated
    by R; differentiable in both.  Returns a NEW tensor (the reference writes in place); a tensor with <= 1 row is returned
    unchanged.  GPU fp32 only, as every operator here."""
    assert shs_feat.shape[-1] == 3, f"SH features must be in RGB format (N, SHS_NUM, 3), but got {tuple(shs_feat.shape)}"
    if shs_feat.shape[1] <= 1:
        return shs_feat
    _rest_degree(shs_feat)
    assert rotation_matrix.shape == (3, 3), f"Rotation matrix must have shape (3, 3), but got {rotation_matrix.shape}."
    L.ptr(shs_feat.detach().contiguous(), torch.float32)            # raises for a CPU / non-fp32 tensor: no fallback
    return _ShRotate.apply(shs_feat, rotation_matrix.to(shs_feat))


def transform_shs_by_quat(shs_feat: Tensor, quaternion: Tensor) -> Tensor:
    """transform_utils.py:25-38 (wxyz)."""
    from ..regist import quat_to_rotmat
    return transform_shs_by_rotmat(shs_feat, quat_to_rotmat(quaternion))


def quaternion_multiply(q0: Tensor, q1: Tensor) -> Tensor:
    """transform_utils.py:14-23"""
    from ..regist import quaternion_multiply as qm
    return qm(q0, q1)


def rotate_transform(points: Tensor, point_rotations: Tensor, rotation_matrix: Tensor):
    """transform_utils.py:201-221: (points @ R.T, normalize(quaternion_multiply(rotations, quat(R)))); the SH coefficients
    are not touched."""
    from ..regist import rotmat_to_quat
    assert rotation_matrix.shape == (3, 3), f"Rotation matrix must have shape (3, 3), but got {rotation_matrix.shape}."
    quat = rotmat_to_quat(rotation_matrix)[None, ...]
    rot = torch.nn.functional.normalize(quaternion_multiply(point_rotations, quat), p=2, dim=-1)
    return points @ rotation_matrix.T, rot


def _touch(gaussians) -> None:
    cache = getattr(gaussians, "_cov_cache", None)
    if cache is not None:
        cache.clear()          # covariances depend on _scaling and _rotation


def translate_gaussians(gaussians, translation: torch.Tensor) -> None:
    """transform_utils.py:107-116"""
    assert translation.shape == (3,), f"Translation vector must have shape (3,), but got {translation.shape}."
    gaussians._xyz = gaussians._xyz + translation.unsqueeze(0).to(gaussians._xyz)


def scale_gaussians(gaussians, scale: Union[torch.Tensor, float], origin: Optional[torch.Tensor] = None) -> None:
    """transform_utils.py:119-137: positions scaled about `origin` (default: centroid) AND MOVED TO IT (the reference
    assigns scale * (xyz - origin), without adding the origin back), log-scales shifted by log(scale)."""
    if isinstance(scale, (float, int)):
        scale = torch.tensor(float(scale), device=gaussians.get_xyz.device, dtype=torch.float32)
    elif isinstance(scale, torch.Tensor):
        assert scale.shape == (1,) or scale.shape == (), f"Scale factor must have shape (1,) or (), but got {scale.shape}."
        scale = scale.to(gaussians.get_xyz)
    else:
        raise ValueError(f"Scale factor must be a torch.Tensor or a float, but got {type(scale)}.")
    if origin is None:
        origin = torch.mean(gaussians.get_xyz, dim=0, keepdim=True)
    gaussians._xyz = scale * (gaussians.get_xyz - origin.to(gaussians.get_xyz))
    gaussians._scaling = gaussians._scaling + torch.log(scale)
    _touch(gaussians)


def rotate_gaussians(gaussians, rotation_matrix: torch.Tensor) -> None:
    """transform_utils.py:140-155: positions, orientations (get_rotation = the normalised quaternions) and the SH
    coefficients above the DC row rotated about the world origin."""
    R = rotation_matrix.to(gaussians.get_xyz)
    gaussians._xyz, gaussians._rotation = rotate_transform(gaussians.get_xyz, gaussians.get_rotation, R)
    gaussians._features_rest = transform_shs_by_rotmat(gaussians._features_rest, R)
    _touch(gaussians)
