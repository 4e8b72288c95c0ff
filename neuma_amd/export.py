"""A rolled-out frame as a standard 3DGS parameter set: what the frame loop holds on the device (means3D, the bound deformation
gradients, optionally the rotated SH coefficients) turned back into (xyz, f_dc, f_rest, opacity, log-scale, quaternion), the only
thing the 3DGS viewers and tools read.  The portable counterpart of the reference's interactive viewer (modules/vis), which this
project does not have: a saved sequence can be looked at from any camera, at any resolution, over any background
(`python -m neuma_amd.replay`), without running the roll-out again.

    deformed_gaussians(gaussians, means3D, deform_grad, shs, scaling_modifier) -> GaussianModel      nm_gaussian_deform, on the GPU
    save_frame(path, ...)                                                                             ... -> io.save_gaussians_ply

The scale modifier is baked into the scales, so a file shows in a foreign viewer what was rendered here and the objects of a
multi-object scene (each with its own modifier) share one file (`concat_gaussians`).  The log-scale of the file format is the
precision bottleneck: nothing here is more accurate than about 1e-6 of the covariance.

GPU tensors go through the kernel and nothing else; a model that lives on the CPU is exported by `save_frame` through
extras/gaussian_export.py (numpy fp64), the kernel's yardstick."""
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L
from .io import save_gaussians_ply
from .render.gaussian_model import GaussianModel


def gaussian_deform(log_scales: Tensor, rot: Tensor, F: Optional[Tensor] = None, scale_modifier: float = 1.0):
    """nm_gaussian_deform on contiguous fp32 GPU tensors log_scales (K,3), rot (K,4), F (K,3,3) or None (identity):
    (log_scales' (K,3), rot' (K,4) unit with r >= 0) whose activation at modifier 1 is F Sigma F^T."""
    dev = L.same_device(log_scales, rot, F)
    K = log_scales.shape[0]
    if tuple(log_scales.shape) != (K, 3) or tuple(rot.shape) != (K, 4) or (F is not None and tuple(F.shape) != (K, 3, 3)):
        raise ValueError(f"log_scales (K,3), rot (K,4), F (K,3,3) expected, got {tuple(log_scales.shape)}, {tuple(rot.shape)}, "
                         f"{None if F is None else tuple(F.shape)}")
    f32 = torch.float32
    p = [L.ptr(log_scales, f32), L.ptr(rot, f32), L.ptr(F, f32)]            # (raises on CPU tensors)
    ls_out = torch.empty(K, 3, dtype=f32, device=dev)
    rot_out = torch.empty(K, 4, dtype=f32, device=dev)
    L.check(L.lib().nm_gaussian_deform(K, p[0], p[1], p[2], float(scale_modifier), L.ptr(ls_out), L.ptr(rot_out), L.stream_ptr(dev)),
            "nm_gaussian_deform")
    return ls_out, rot_out


def _rest(gaussians, shs: Optional[Tensor]) -> Tensor:
    if shs is None:
        return gaussians._features_rest
    n = gaussians._features_dc.shape[1] + gaussians._features_rest.shape[1]
    if shs.dim() != 3 or shs.shape[0] != gaussians._xyz.shape[0] or shs.shape[1] != n or shs.shape[2] != 3:
        raise ValueError(f"shs must be (K, {n}, 3) like the model's get_features, got {tuple(shs.shape)}")
    return shs[:, 1:].detach().contiguous()


@torch.no_grad()
def deformed_gaussians(gaussians, means3D: Tensor, deform_grad: Optional[Tensor] = None, shs: Optional[Tensor] = None,
                       scaling_modifier: float = 1.0) -> GaussianModel:
    """The frame (means3D (K,3), deform_grad (K,3,3) or (K,9) or None) of `gaussians` as a new GaussianModel on the same device.
    _opacity and _features_dc are the input's own tensors; _features_rest too, unless `shs` (K,n,3) carries the coefficients the
    frame was rendered with (rotate_sh), whose rows 1.. are taken.  Raises on CPU tensors and on a non-finite deform_grad (one
    host read-back per exported frame)."""
    if not (means3D.is_cuda and gaussians._scaling.is_cuda):
        raise L.NeumaHipError("deformed_gaussians needs tensors on the GPU (CPU models: save_frame / extras.gaussian_export)")
    K = gaussians._scaling.shape[0]
    if tuple(means3D.shape) != (K, 3):
        raise ValueError(f"means3D must be ({K}, 3), got {tuple(means3D.shape)}")
    F = None
    if deform_grad is not None:
        F = deform_grad.detach().float().reshape(-1, 3, 3).contiguous()
        if F.shape[0] != K:
            raise ValueError(f"{F.shape[0]} deformation gradients for {K} Gaussians")
        if not bool(torch.isfinite(F).all()):
            raise ValueError("deform_grad holds non-finite values")
    ls, rot = gaussian_deform(gaussians._scaling.detach().float().contiguous(), gaussians._rotation.detach().float().contiguous(), F,
                              scaling_modifier)
    out = GaussianModel(gaussians.max_sh_degree)
    out.active_sh_degree = gaussians.active_sh_degree
    return out.set_params(means3D.detach(), gaussians._features_dc, _rest(gaussians, shs), ls, rot, gaussians._opacity)


def concat_gaussians(models: Sequence[GaussianModel]) -> GaussianModel:
    """One model of several (the objects of a scene, in order); they share one SH degree."""
    assert len(models) > 0 and all(m.max_sh_degree == models[0].max_sh_degree for m in models), "objects differ in SH degree"
    if len(models) == 1:
        return models[0]
    out = GaussianModel(models[0].max_sh_degree)
    out.active_sh_degree = models[0].active_sh_degree
    cat = lambda attr: torch.cat([getattr(m, attr).detach() for m in models], 0)
    return out.set_params(cat("_xyz"), cat("_features_dc"), cat("_features_rest"), cat("_scaling"), cat("_rotation"), cat("_opacity"))


@torch.no_grad()
def save_frame(path, gaussians, means3D: Tensor, deform_grad: Optional[Tensor] = None, shs: Optional[Tensor] = None,
               scaling_modifier: float = 1.0) -> GaussianModel:
    """deformed_gaussians(...) written with io.save_gaussians_ply: exactly the properties, in the order, of kernels.ply.  A model
    and frame on the CPU take the numpy fp64 path of extras/gaussian_export.py.  Returns the model it wrote."""
    if means3D.is_cuda or gaussians._scaling.is_cuda:
        model = deformed_gaussians(gaussians, means3D, deform_grad, shs, scaling_modifier)
    else:
        from .extras.gaussian_export import deformed_parameters
        _rest(gaussians, shs)                                               # (shape check)
        model = deformed_parameters(gaussians, means3D.detach(), deform_grad, None if shs is None else shs.detach(), scaling_modifier)
    save_gaussians_ply(model, path)
    return model
