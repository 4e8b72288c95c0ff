"""`python -m neuma_amd.regist -c <regist-*.yaml>` - the first stage of NeuMA's real-world pipeline: fit one rotation, one
translation and one uniform scale that move a reconstructed Gaussian set onto the first video frame, then move the mesh-sampled
particles by the same transform.  Counterpart of /root/reference/experiments/regist.py (regist_gaussians 50-205,
regist_particles 208-247, transform_pcd 40-47) and modules/tune/regist/register.py (Register).

Outputs in <assets_root>/<sim_data_name>/ (what finetune-<obj>.yaml points at):
    registered_params.npz     r (3x3), t (3,), s (1,), o (1,3)
    registered_kernels.ply    the transformed Gaussians
    registered_particles.ply  transform_pcd(sample_mesh_points(mesh))

Per iteration the reference runs the transform in torch autograd, 3 renders forward + backward, l1 + lambda (1 - ssim) and a
`loss.item()`.  Here (NativeRegistration): nm_regist_apply, per view raster_forward_raw -> nm_pixel_loss -> nm_ssim_loss ->
raster_backward_raw -> nm_regist_backward into 17 device scalars (dR, dq_R, ds, dt), torch autograd from those to r, t, s only,
RAdam + the cosine schedule; the loss goes to a device history that is read at the end.  With sh_degree > 0 the colour
coefficients turn with the Gaussians (register.py:68-91, transform_shs_by_quat): one nm_sh_rotate per iteration with the R the
loop already packed, and per view nm_sh_rotate_backward adds the colour gradient's share into the same dR.  `regist_step_torch`
is the same iteration through the differentiable torch path (build_cov3D + GaussianRasterizer + tune.ssim +
transform_utils.rotate_shs_torch).

Rotation conversions follow pytorch3d.transforms' published conventions (wxyz quaternions, Gram-Schmidt 6D rows, the
best-conditioned candidate of matrix_to_quaternion, standardised to a non-negative real part)."""
import argparse
import random
import sys
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _lib as L

# ------------------------------------------------------------------ rotation conversions (pytorch3d.transforms conventions)


def rot6d_to_rotmat(d6: Tensor) -> Tensor:
    """rotation_6d_to_matrix: Gram-Schmidt on the two 3-vectors; they become the matrix ROWS."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def rotmat_to_rot6d(m: Tensor) -> Tensor:
    """matrix_to_rotation_6d: the first two rows."""
    return m[..., :2, :].clone().reshape(m.shape[:-2] + (6,))


def quat_to_rotmat(q: Tensor) -> Tensor:
    """quaternion_to_matrix (wxyz, need not be unit)."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _sqrt_positive_part(x: Tensor) -> Tensor:
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def rotmat_to_quat(m: Tensor) -> Tensor:
    """matrix_to_quaternion: four candidates, the one divided by the largest |q_i| (floor 0.1) is taken; then
    standardize_quaternion (real part >= 0).  Differentiable (the selection is a gather)."""
    batch = m.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m.reshape(batch + (9,)), -1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22,
                                             1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1))
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    idx = q_abs.argmax(-1)
    out = cand.gather(-2, idx[..., None, None].expand(batch + (1, 4))).squeeze(-2)
    return torch.where(out[..., 0:1] < 0, -out, out)


def _axis_rotation(axis: str, angle: Tensor) -> Tensor:
    c, s = torch.cos(angle), torch.sin(angle)
    one, zero = torch.ones_like(angle), torch.zeros_like(angle)
    if axis == "X":
        flat = (one, zero, zero, zero, c, -s, zero, s, c)
    elif axis == "Y":
        flat = (c, zero, s, zero, one, zero, -s, zero, c)
    else:
        flat = (c, -s, zero, s, c, zero, zero, zero, one)
    return torch.stack(flat, -1).reshape(angle.shape + (3, 3))


def euler_to_rotmat(euler: Tensor, convention: str = "XYZ") -> Tensor:
    """euler_angles_to_matrix (radians): R = R_c0(e0) R_c1(e1) R_c2(e2)."""
    mats = [_axis_rotation(c, e) for c, e in zip(convention, torch.unbind(euler, -1))]
    return mats[0] @ mats[1] @ mats[2]


def euler_to_quat(euler: Tensor, convention: str = "XYZ") -> Tensor:
    return rotmat_to_quat(euler_to_rotmat(euler, convention))


def rotmat_to_euler_xyz(m: Tensor) -> Tensor:
    """matrix_to_euler_angles(m, "XYZ"): (atan2(-m12, m22), asin(m02), atan2(-m01, m00))."""
    return torch.stack((torch.atan2(-m[..., 1, 2], m[..., 2, 2]), torch.asin(m[..., 0, 2].clamp(-1.0, 1.0)),
                        torch.atan2(-m[..., 0, 1], m[..., 0, 0])), -1)


def quat_to_euler(q: Tensor, convention: str = "XYZ") -> Tensor:
    if convention != "XYZ":
        raise NotImplementedError("quat_to_euler: only the XYZ convention (the one Register uses)")
    return rotmat_to_euler_xyz(quat_to_rotmat(q))


def quat_to_rot6d(q: Tensor) -> Tensor:
    return rotmat_to_rot6d(quat_to_rotmat(q))


def rot6d_to_quat(d6: Tensor) -> Tensor:
    return rotmat_to_quat(rot6d_to_rotmat(d6))


def quaternion_multiply(q0: Tensor, q1: Tensor) -> Tensor:
    """transform_utils.py:14-23 (this operand order)."""
    w0, x0, y0, z0 = torch.unbind(q0, -1)
    w1, x1, y1, z1 = torch.unbind(q1, -1)
    return torch.stack((-x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0, x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0,
                        -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0, x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0), -1)


def transform_pcd(points, scale, origin, rotation, translation):
    """regist.py:40-47 (numpy)."""
    points = (np.asarray(points) - origin) * scale
    points = np.dot(points, np.asarray(rotation).T)
    return points + translation


# ------------------------------------------------------------------ Register


class Register(nn.Module):
    """register.py: r (6D rotation), t (3,), s (1,); RAdam (eps 1e-15) with per-group lr_r / lr_t / lr_s and the cosine
    schedule through LambdaLR."""

    def __init__(self, cfg, device="cuda"):
        super().__init__()
        self.cfg = cfg
        euler = torch.tensor(cfg["INIT_R"], dtype=torch.float32, device=device) * torch.pi / 180
        self.r = nn.Parameter(quat_to_rot6d(euler_to_quat(euler)), requires_grad=True)
        self.t = nn.Parameter(torch.tensor(cfg["INIT_T"], dtype=torch.float32, device=device), requires_grad=True)
        self.s = nn.Parameter(torch.tensor(cfg["INIT_S"], dtype=torch.float32, device=device), requires_grad=True)

    def training_setup(self):
        from .train import CosineDecayScheduler
        groups = [{"params": [self.r], "lr": self.cfg["lr_r"], "name": "r"},
                  {"params": [self.t], "lr": self.cfg["lr_t"], "name": "t"},
                  {"params": [self.s], "lr": self.cfg["lr_s"], "name": "s"}]
        self.optimizer = torch.optim.RAdam(groups, lr=0.0, eps=1e-15)
        self.scheduler = CosineDecayScheduler(self.cfg["scheduler"]).get_scheduler(self.optimizer, 0.0)

    @property
    def get_scale(self):
        return self.s

    @property
    def get_quat(self):
        return rot6d_to_quat(self.r)

    @property
    def get_euler(self):
        return torch.rad2deg(quat_to_euler(rot6d_to_quat(self.r)))

    @property
    def get_rotmat(self):
        return rot6d_to_rotmat(self.r)

    def forward(self, points: Tensor, scales: Tensor, rotations: Tensor, scaling_modifier: float = 1.0,
                f_rest: Optional[Tensor] = None):
        """register.py forward (points / log-scales / quaternions as loaded) + the covariance build, differentiable in r, t,
        s.  Returns points, scales (log), rotations (normalised), cov3D (K,6) and origin (1,3); with `f_rest` (K, 3|8|15, 3)
        also "f_rest", the SH coefficients above the DC row rotated by the same R (register.py:85, differentiable in r)."""
        from .render import build_cov3D
        R = rot6d_to_rotmat(self.r)
        q_R = rotmat_to_quat(R)
        origin = points.detach().mean(0, keepdim=True)
        pts = self.s * (points.detach() - origin)
        ls = scales.detach() + torch.log(self.s)
        pts = pts @ R.T
        rot = F.normalize(quaternion_multiply(F.normalize(rotations.detach(), dim=-1), q_R[None]), p=2, dim=-1)
        pts = pts + self.t[None]
        cov = build_cov3D(torch.exp(ls), rot, scaling_modifier)
        out = {"points": pts, "scales": ls, "rotations": rot, "cov3D": cov, "origin": origin}
        if f_rest is not None:
            from .render.transform_utils import rotate_shs_torch
            out["f_rest"] = rotate_shs_torch(f_rest.detach(), R)
        return out


def pack_params(register: Register, origin: Tensor):
    """(R (3,3), q_R (4,), device params (20,) = R[9], q_R[4], s, t[3], o[3]) - a few torch ops, no host sync."""
    R = rot6d_to_rotmat(register.r)
    q_R = rotmat_to_quat(R)
    params = torch.cat([R.reshape(9), q_R, register.s.reshape(1), register.t.reshape(3), origin.reshape(3)]).detach().contiguous()
    return R, q_R, params


def regist_apply(xyz: Tensor, log_scales: Tensor, rot: Tensor, params: Tensor, scale_modifier: float = 1.0,
                 want_params: bool = False):
    """nm_regist_apply: (means3D (K,3), cov6 (K,6)[, log_scales' (K,3), rot' (K,4)])."""
    K = xyz.shape[0]
    dev = xyz.device
    means3D = torch.empty(K, 3, dtype=torch.float32, device=dev)
    cov6 = torch.empty(K, 6, dtype=torch.float32, device=dev)
    ls = torch.empty(K, 3, dtype=torch.float32, device=dev) if want_params else None
    rq = torch.empty(K, 4, dtype=torch.float32, device=dev) if want_params else None
    L.check(L.lib().nm_regist_apply(K, L.ptr(xyz), L.ptr(log_scales), L.ptr(rot), L.ptr(params), float(scale_modifier), L.ptr(means3D),
                                    L.ptr(cov6), L.ptr(ls), L.ptr(rq), L.stream_ptr(dev)), "nm_regist_apply")
    return (means3D, cov6, ls, rq) if want_params else (means3D, cov6)


def regist_backward(xyz, log_scales, rot, params, scale_modifier, dmeans3D, dcov6, dparams: Tensor, workspace: Optional[Tensor] = None):
    """nm_regist_backward: dparams (17,) += (dR[9], dq_R[4], ds, dt[3]) reduced over the Gaussians."""
    lib = L.lib()
    K = xyz.shape[0]
    nbytes = int(lib.nm_regist_bwd_workspace(K))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
    L.check(lib.nm_regist_backward(K, L.ptr(xyz), L.ptr(log_scales), L.ptr(rot), L.ptr(params), float(scale_modifier), L.ptr(dmeans3D),
                                   L.ptr(dcov6), L.ptr(dparams), L.ptr(workspace), workspace.numel(), L.stream_ptr(xyz.device)),
            "nm_regist_backward")
    return dparams


def params_backward(register: Register, R: Tensor, q_R: Tensor, dparams: Tensor) -> None:
    """torch autograd from the 17 reduced scalars to r, t, s (the r6 -> R -> q_R chain on 10 scalars)."""
    torch.autograd.backward([R.reshape(9), q_R, register.s, register.t],
                            [dparams[0:9], dparams[9:13], dparams[13:14].reshape(register.s.shape), dparams[14:17]])


_PIXEL_KIND = {"l1": 0, "l2": 1}


class NativeRegistration(object):
    """The registration loop on the HIP operators.  gaussians: a GaussianModel as loaded; cameras: objects get_rasterizer
    accepts (one per used view, the first step's); gts: (3,H,W) images.  step() enqueues one iteration and returns nothing;
    `losses()` reads the device loss history (one host sync)."""

    def __init__(self, register: Register, gaussians, cameras: Sequence, gts: Sequence[Tensor], background: Tensor,
                 lambda_ssim: float = 0.0, pixel_loss: str = "l1", scaling_modifier: float = 1.0, force_mask_data: bool = False,
                 num_iter: int = 1):
        from .render import RasterCamera, get_rasterizer
        self.reg = register
        dev = gaussians.get_xyz.device
        self.dev = dev
        self.xyz = gaussians._xyz.detach().float().contiguous()
        self.ls = gaussians._scaling.detach().float().contiguous()
        self.rot = gaussians._rotation.detach().float().contiguous()
        self.K = self.xyz.shape[0]
        self.origin = self.xyz.mean(0, keepdim=True)
        self.op = gaussians.get_opacity.detach().float().contiguous()
        if force_mask_data:
            self.sh, self.cp = None, torch.ones(self.K, 3, dtype=torch.float32, device=dev)
        else:
            self.sh, self.cp = gaussians.get_features.detach().float().contiguous(), None
        sh_degree = gaussians.active_sh_degree
        # sh_degree > 0: the coefficients above the DC row turn with the Gaussians; self.sh stays as loaded, the renders read
        # self.sh_rot (written once per iteration)
        self.rotate_sh = self.sh is not None and sh_degree > 0 and self.sh.shape[1] > 1
        self.sh_rot = torch.empty_like(self.sh) if self.rotate_sh else None
        rest = gaussians._features_rest
        self.f_rest = rest.detach().float().contiguous() if sh_degree > 0 and rest.dim() == 3 and rest.shape[1] > 0 else None
        self.cams: List[RasterCamera] = [get_rasterizer(c, sh_degree, False, background)._cam for c in cameras]
        self.gts = [g.detach().to(dev).float().contiguous() for g in gts]
        self.lam = float(lambda_ssim)
        self.kind = _PIXEL_KIND[pixel_loss]
        self.mod = float(scaling_modifier)
        lib = L.lib()
        self.loss_hist = torch.zeros(max(int(num_iter), 1), dtype=torch.float32, device=dev)
        self.dparams = torch.zeros(17, dtype=torch.float32, device=dev)
        self.ws_reg = torch.empty(int(lib.nm_regist_bwd_workspace(self.K)), dtype=torch.uint8, device=dev)
        self.ws_shrot = torch.empty(int(lib.nm_sh_rotate_bwd_workspace(self.K)), dtype=torch.uint8, device=dev) if self.rotate_sh else None
        self.ws_ssim = {}
        self.n = 0
        self.last_renders: List[Tensor] = []
        self.last_params: Optional[Tensor] = None

    def _ssim_ws(self, h, w):
        key = (h, w)
        if key not in self.ws_ssim:
            self.ws_ssim[key] = torch.empty(int(L.lib().nm_ssim_workspace(h, w)), dtype=torch.uint8, device=self.dev)
        return self.ws_ssim[key]

    def step(self, keep_renders: bool = False) -> None:
        from .render import raster_backward_raw, raster_forward_raw
        lib = L.lib()
        reg = self.reg
        if self.n >= self.loss_hist.numel():
            self.loss_hist = torch.cat([self.loss_hist, torch.zeros_like(self.loss_hist)])
        loss = self.loss_hist[self.n]
        stream = L.stream_ptr(self.dev)
        R, q_R, params = pack_params(reg, self.origin)
        means3D, cov6 = regist_apply(self.xyz, self.ls, self.rot, params, self.mod)
        self.dparams.zero_()
        self.last_renders = []
        sh = self.sh
        if self.rotate_sh:
            sh = self._rotated_sh(params)
        for cam, gt in zip(self.cams, self.gts):
            color, _, rec = raster_forward_raw(cam, means3D, sh, self.cp, self.op, cov6)
            h, w = int(color.shape[-2]), int(color.shape[-1])
            gimg = torch.empty_like(color)
            L.check(lib.nm_pixel_loss(self.kind, 1.0 - self.lam, h, w, 0, 0, L.ptr(color), L.ptr(gt), L.ptr(loss), L.ptr(gimg), stream),
                    "nm_pixel_loss")
            if self.lam > 0:
                ws = self._ssim_ws(h, w)
                L.check(lib.nm_ssim_loss(self.lam, h, w, L.ptr(color), L.ptr(gt), L.ptr(loss), L.ptr(gimg), L.ptr(ws), ws.numel(), stream),
                        "nm_ssim_loss")
            dm, _, dcov, _, dsh, _ = raster_backward_raw(rec, gimg, need_cov=True, need_color=self.rotate_sh)
            regist_backward(self.xyz, self.ls, self.rot, params, self.mod, dm, dcov, self.dparams, self.ws_reg)
            if self.rotate_sh:                                            # dparams[0:9] (dR) += the colours' share
                L.check(lib.nm_sh_rotate_backward(self.K, self.sh.shape[1], 1, L.ptr(params), L.ptr(self.sh), L.ptr(dsh),
                                                  L.ptr(self.dparams), None, L.ptr(self.ws_shrot), self.ws_shrot.numel(), stream),
                        "nm_sh_rotate_backward")
            if keep_renders:
                self.last_renders.append(color)
        params_backward(reg, R, q_R, self.dparams)
        self.last_params = params
        reg.optimizer.step()
        reg.optimizer.zero_grad(set_to_none=True)
        reg.scheduler.step()
        self.n += 1

    def _rotated_sh(self, params: Tensor) -> Tensor:
        """self.sh_rot <- diag(1, D(R)) self.sh with R = params[0:9], on the device (nothing is read back)."""
        L.check(L.lib().nm_sh_rotate(self.K, self.sh.shape[1], 1, L.ptr(params), L.ptr(self.sh), L.ptr(self.sh_rot),
                                     L.stream_ptr(self.dev)), "nm_sh_rotate")
        return self.sh_rot

    def losses(self) -> np.ndarray:
        return self.loss_hist[:self.n].double().cpu().numpy()

    def transformed(self, with_f_rest: bool = False):
        """(means3D, log-scales, rotations) under the transform the LAST iteration rendered with (regist.py:204 saves the
        Gaussians of the last forward pass, i.e. one optimizer step behind registered_params.npz), through nm_regist_apply.
        with_f_rest: a fourth entry, the SH coefficients above the DC row under the same transform through nm_sh_rotate (None
        at sh_degree 0)."""
        params = self.last_params if self.last_params is not None else pack_params(self.reg, self.origin)[2]
        m, _, ls, rq = regist_apply(self.xyz, self.ls, self.rot, params, self.mod, want_params=True)
        if not with_f_rest:
            return m, ls, rq
        from .render.transform_utils import sh_rotate
        return m, ls, rq, (sh_rotate(self.f_rest, params[0:9], False) if self.f_rest is not None else None)


def ema_of(losses) -> float:
    """regist.py:177: ema = 0.4 loss + 0.6 ema over the whole history, from 0."""
    ema = 0.0
    for v in losses:
        ema = 0.4 * float(v) + 0.6 * ema
    return ema


def regist_step_torch(register: Register, gaussians, cameras: Sequence, gts: Sequence[Tensor], background: Tensor,
                      lambda_ssim: float = 0.0, pixel_loss: str = "l1", scaling_modifier: float = 1.0,
                      force_mask_data: bool = False, step_optimizer: bool = True):
    """One iteration of regist.py:143-203 through torch autograd (the differentiable path: Register.forward, build_cov3D, the
    GaussianRasterizer autograd op, tune.l1_loss / l2_loss / ssim).  Returns (loss tensor, renders)."""
    from .render import get_rasterizer
    from .tune import l1_loss, l2_loss, ssim
    pix = {"l1": l1_loss, "l2": l2_loss}[pixel_loss]
    rotate_sh = (not force_mask_data) and gaussians.active_sh_degree > 0 and gaussians._features_rest.shape[1] > 0
    pack = register(gaussians._xyz, gaussians._scaling, gaussians._rotation, scaling_modifier,
                    f_rest=gaussians._features_rest if rotate_sh else None)
    shs = torch.cat((gaussians._features_dc.detach(), pack["f_rest"]), dim=1) if rotate_sh else gaussians.get_features.detach()
    op = gaussians.get_opacity.detach()
    K = pack["points"].shape[0]
    loss = 0.0
    renders = []
    for cam, gt in zip(cameras, gts):
        rast = get_rasterizer(cam, gaussians.active_sh_degree, False, background)
        means2D = torch.zeros_like(pack["points"])
        if force_mask_data:
            img, _ = rast(means3D=pack["points"], means2D=means2D, opacities=op, shs=None,
                          colors_precomp=torch.ones(K, 3, device=op.device), cov3D_precomp=pack["cov3D"])
        else:
            img, _ = rast(means3D=pack["points"], means2D=means2D, opacities=op, shs=shs,
                          colors_precomp=None, cov3D_precomp=pack["cov3D"])
        gt = gt.to(img.device)
        loss = loss + (1.0 - lambda_ssim) * pix(img, gt)
        if lambda_ssim > 0:
            loss = loss + lambda_ssim * (1.0 - ssim(img, gt))
        renders.append(img)
    if step_optimizer:
        loss.backward()
        register.optimizer.step()
        register.optimizer.zero_grad(set_to_none=True)
        register.scheduler.step()
    return loss, renders


# ------------------------------------------------------------------ entry point


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", "-c", type=str, required=True, help="Path to the config file.")
    return p.parse_args(argv)


def _assets_root(cfg) -> Path:
    return Path(cfg.get("assets_root", "experiments/assets"))


def _save_debug_grid(renders: List[Tensor], gts: List[Tensor], path) -> None:
    """torchvision save_image(cat[renders, gts], nrow=len(views)) of the regist.py:160-200 crop [:, 100:500, 720:1100]
    (padding 2, black)."""
    from .evaluate import save_image
    def crop(t):
        c = t.detach().to(renders[0].device)[:, 100:500, 720:1100]
        return c if c.numel() else t.detach().to(renders[0].device)        # (images smaller than the crop: the whole image)
    crops = [crop(t) for t in renders] + [crop(t) for t in gts]
    n = len(renders)
    h, w = crops[0].shape[-2:]
    pad = 2
    grid = torch.zeros(3, pad + 2 * (h + pad), pad + n * (w + pad), device=crops[0].device)
    for idx, c in enumerate(crops):
        r, k = divmod(idx, n)
        grid[:, pad + r * (h + pad): pad + r * (h + pad) + c.shape[-2], pad + k * (w + pad): pad + k * (w + pad) + c.shape[-1]] = c
    save_image(grid, path)


def regist_gaussians(cfg, log=print) -> Optional[float]:
    """regist.py:50-205.  Returns the final EMA loss (None when the stage is skipped)."""
    from . import io as nio
    from .config import save_config
    from .dataset import VideoDataset
    data_root = _assets_root(cfg) / cfg.sim_data_name
    data_root.mkdir(parents=True, exist_ok=True)
    if (data_root / "registered_params.npz").is_file() and (data_root / "registered_kernels.ply").is_file():
        log("===================================")
        log("Registration for Gaussians already finished. Skip.\n")
        log("\nRegistration finished.")
        log("===================================")
        return None
    log("\n===================================")
    log("Registering Gaussian kernels ...\n")
    seed = cfg.seed
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    debug = bool(cfg.get("debug", False))
    device = torch.device(f"cuda:{cfg.gpu}")
    torch.cuda.set_device(device)
    force_mask_data = bool(cfg.video_data.data.get("read_mask_only", False))
    if force_mask_data:
        cfg.video_data.data.white_background = False
        log("[Warning] Force to use black background when loading mask data")
    background = torch.tensor([1.0, 1.0, 1.0] if cfg.video_data.data.get("white_background", False) else [0.0, 0.0, 0.0],
                              dtype=torch.float32, device=device)
    gaussians = nio.load_gaussians_ply(cfg.gaussian.kernels_path, cfg.gaussian.sh_degree, device=device)
    rotate_sh = cfg.gaussian.sh_degree > 0 and gaussians._features_rest.numel() > 0
    if rotate_sh and not bool(cfg.register.get("rotate_sh", False)):
        raise NotImplementedError("registration of Gaussians with sh_degree > 0 rotates the SH coefficients with the Gaussians "
                                  "(transform_shs_by_quat); it is opt-in: set `register.rotate_sh: true` in the config")
    save_config(cfg, data_root / "config.yaml")
    debug_root = data_root / "debug"
    if debug:
        debug_root.mkdir(exist_ok=True)
    cfg.video_data.device = str(device)                                   # NOTE: manually setting (regist.py:100)
    dataset = VideoDataset(cfg.video_data)
    rc = cfg.register
    used_views = sorted(dataset.views if rc.get("views", "all") == "all" else rc.views)
    first_step = dataset.steps[0]
    pixel_loss = rc.get("pixel_loss", "l1")
    lam = float(rc.get("lambda_ssim_loss", 0.0))
    log(f"[register] Using views: {used_views}")
    log(f"[register] Using first step: {first_step}")
    log(f"[register] Using pixel loss: {pixel_loss}")
    log(f"[register] Lambda ssim loss: {lam}")
    log("[register] Training register ...")
    register = Register(rc, device=device)
    register.training_setup()
    cams = [dataset.getCameras(v, first_step) for v in used_views]
    gts = [c.original_image.to(device) for c in cams]
    num_iter = int(rc.num_iter)
    run = NativeRegistration(register, gaussians, cams, gts, background, lambda_ssim=lam, pixel_loss=pixel_loss,
                             scaling_modifier=cfg.gaussian.get("scaling_modifier", 1.0), force_mask_data=force_mask_data,
                             num_iter=num_iter)
    for i in range(1, num_iter + 1):
        dbg = debug and (i == 1 or i % 500 == 0)
        run.step(keep_renders=dbg)
        if dbg:
            _save_debug_grid(run.last_renders, gts, debug_root / f"regist_iter_{i}.png")
        if i % 1000 == 0 or i == num_iter:
            e = register.get_euler.detach().cpu().tolist()
            t = register.t.detach().cpu().tolist()
            log(f"[{i}/{num_iter}] Loss {ema_of(run.losses()):.7f} | r [{e[0]:.2f}, {e[1]:.2f}, {e[2]:.2f}] | "
                f"t [{t[0]:.3f}, {t[1]:.3f}, {t[2]:.3f}] | s {float(register.s.detach()[0]):.4f}")
    ema = ema_of(run.losses())
    np.savez_compressed(data_root / "registered_params.npz", r=register.get_rotmat.detach().cpu().numpy(),
                        t=register.t.detach().cpu().numpy(), s=register.s.detach().cpu().numpy(), o=run.origin.cpu().numpy())
    with torch.no_grad():
        m, ls, rq, f_rest = run.transformed(with_f_rest=True)
    gaussians.set_params(m, gaussians._features_dc, f_rest if f_rest is not None else gaussians._features_rest, ls, rq,
                         gaussians._opacity)
    nio.save_gaussians_ply(gaussians, data_root / "registered_kernels.ply")
    log(f"\nRegistration finished. Loss: {ema:.7f}")
    log("===================================")
    return ema


def regist_particles(cfg, log=print, device=None) -> np.ndarray:
    """regist.py:208-247 with the project's mesh sampler ('surface' needs trimesh: unavailable): mesh_inside on a GPU
    `device` (default cuda:<cfg.gpu>, as regist_gaussians), extras.mesh_sampling otherwise - the same particles."""
    import shutil
    from . import io as nio
    from . import mesh_inside
    from .extras import mesh_sampling as mesh
    device = torch.device(device if device is not None else f"cuda:{cfg.get('gpu', 0)}")
    save_dir = _assets_root(cfg) / cfg.sim_data_name
    out = save_dir / "registered_particles.ply"
    if out.is_file():
        log("\n===================================")
        log("Registration for Particles already finished. Skip.\n")
        pts = nio.load_particles_ply(out)
    else:
        log("\n===================================")
        log("Registering Particles ...\n")
        mesh_path = Path(cfg.particle_data.mesh_path)
        log(f"Extracting particles from mesh file [{mesh_path}] ...")
        shutil.copyfile(mesh_path, save_dir / f"mesh{mesh_path.suffix}")
        reader = mesh.read_obj_mesh if mesh_path.suffix.lower() == ".obj" else mesh.read_ply_mesh
        mode = cfg.particle_data.get("mesh_sample_mode", "volumetric")
        res = int(cfg.particle_data["mesh_sample_resolution"])
        if device.type == "cuda":
            particles = mesh_inside.sample_mesh_points(*reader(mesh_path), mode=mode, resolution=res, device=device)
        else:
            particles = mesh.sample_mesh_points(*reader(mesh_path), mode=mode, resolution=res)
        tr = np.load(save_dir / "registered_params.npz")
        pts = transform_pcd(particles, tr["s"], tr["o"], tr["r"], tr["t"])
        nio.save_particles_ply(out, pts)
    log(f"\nRegistration finished. Registed particles: {pts.shape}")
    log("===================================")
    return pts


def main(argv=None):
    from .config import load_config
    args = parse_args(argv)
    cfg = load_config(args.config)
    regist_gaussians(cfg)
    regist_particles(cfg)


if __name__ == "__main__":
    sys.exit(main())
