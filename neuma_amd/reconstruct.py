"""`python -m neuma_amd.reconstruct -c <finetune or regist yaml> -o <kernels.ply>` - the stage in front of every other one: fit
static 3D Gaussians to the views of one time step, the `kernels.ply` that prepare / regist / finetune start from (the reference
sends its users to the upstream gaussian-splatting repository for it).  The schedule is upstream 3DGS's train.py: L1 +
lambda (1 - SSIM), Adam with the exponential position schedule, SH degree up every 1000 iterations, densification (clone /
split / prune) and opacity resets.

Per iteration (NativeGaussianFit.step), no autograd graph and no host read-back: nm_gaussian_activate -> raster_forward_raw ->
nm_pixel_loss -> nm_ssim_loss -> raster_backward_raw -> nm_gaussian_activate_backward -> the six .grad tensors ->
optimizer.step(); the loss goes to a device history.  `fit_step_torch` is the same iteration through the differentiable torch
path (build_cov3D + the GaussianRasterizer autograd op + tune.l1_loss / ssim + loss.backward())."""
import argparse
import random
import sys
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

DEFAULTS = dict(iterations=30_000, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                position_lr_max_steps=30_000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3,
                percent_dense=0.01, lambda_dssim=0.2, densify_from_iter=500, densify_until_iter=15_000,
                densification_interval=100, opacity_reset_interval=3000, densify_grad_threshold=2e-4)


def fit_options(**overrides) -> SimpleNamespace:
    """The schedule as a namespace: upstream's defaults, every value a keyword."""
    unknown = set(overrides) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown fit options: {sorted(unknown)}")
    return SimpleNamespace(**{**DEFAULTS, **overrides})


def camera_extent(cameras: Sequence) -> float:
    """Upstream's getNerfppNorm radius: the largest distance of a camera centre from the mean centre, x 1.1."""
    c = torch.stack([torch.as_tensor(cam.camera_center).detach().double().cpu().reshape(3) for cam in cameras])
    return float((c - c.mean(0, keepdim=True)).norm(dim=1).max()) * 1.1


class NativeGaussianFit(object):
    """One training iteration on the HIP operators.  gaussians: a GaussianModel after training_setup(); background: (3,) on
    the device.  step() enqueues the iteration and returns (radii, dL/dmeans2D) for the densification statistics; `losses()`
    reads the device loss history (one host sync)."""

    def __init__(self, gaussians, background: Tensor, lambda_dssim: float = 0.2, num_iter: int = 1):
        self.g = gaussians
        self.dev = gaussians.get_xyz.device
        self.background = background
        self.lam = float(lambda_dssim)
        self.loss_hist = torch.zeros(max(int(num_iter), 1), dtype=torch.float32, device=self.dev)
        self.n = 0
        self._cams = {}
        self._ws_ssim = {}

    def _raster_camera(self, camera):
        from .render import get_rasterizer
        key = (id(camera), self.g.active_sh_degree)
        if key not in self._cams:
            self._cams[key] = (camera, get_rasterizer(camera, self.g.active_sh_degree, False, self.background)._cam)
        return self._cams[key][1]

    def step(self, camera, gt_image: Tensor, keep_render: bool = False):
        from .render import gaussian_activate, gaussian_activate_backward, raster_backward_raw, raster_forward_raw
        lib = L.lib()
        g = self.g
        if self.n >= self.loss_hist.numel():
            self.loss_hist = torch.cat([self.loss_hist, torch.zeros_like(self.loss_hist)])
        loss = self.loss_hist[self.n]
        stream = L.stream_ptr(self.dev)
        xyz, ls, rot, logit = g._xyz.detach(), g._scaling.detach(), g._rotation.detach(), g._opacity.detach()
        cov6, op = gaussian_activate(ls, rot, logit, 1.0)
        sh = g.get_features.detach().contiguous()
        color, radii, rec = raster_forward_raw(self._raster_camera(camera), xyz, sh, None, op, cov6)
        h, w = int(color.shape[-2]), int(color.shape[-1])
        gimg = torch.empty_like(color)
        L.check(lib.nm_pixel_loss(0, 1.0 - self.lam, h, w, 0, 0, L.ptr(color), L.ptr(gt_image), L.ptr(loss), L.ptr(gimg), stream),
                "nm_pixel_loss")
        if self.lam > 0:
            if (h, w) not in self._ws_ssim:
                self._ws_ssim[(h, w)] = torch.empty(int(lib.nm_ssim_workspace(h, w)), dtype=torch.uint8, device=self.dev)
            ws = self._ws_ssim[(h, w)]
            L.check(lib.nm_ssim_loss(self.lam, h, w, L.ptr(color), L.ptr(gt_image), L.ptr(loss), L.ptr(gimg), L.ptr(ws), ws.numel(),
                                     stream), "nm_ssim_loss")
        dxyz, dm2, dcov, dop, dsh, _ = raster_backward_raw(rec, gimg, need_means2D=True, need_cov=True, need_opacity=True,
                                                           need_color=True)
        dls, drot, dlogit = gaussian_activate_backward(ls, rot, logit, 1.0, dcov, dop)
        g._xyz.grad, g._scaling.grad, g._rotation.grad, g._opacity.grad = dxyz, dls, drot, dlogit
        g._features_dc.grad = dsh[:, :1].contiguous()
        g._features_rest.grad = dsh[:, 1:].contiguous()
        g.optimizer.step()
        g.optimizer.zero_grad(set_to_none=True)
        g.invalidate()
        self.n += 1
        self.last_render = color if keep_render else None
        return radii, dm2

    def losses(self) -> np.ndarray:
        return self.loss_hist[:self.n].double().cpu().numpy()


def fit_step_torch(gaussians, camera, gt_image: Tensor, background: Tensor, lambda_dssim: float = 0.2, step_optimizer: bool = True):
    """The same iteration through torch autograd.  Returns (loss tensor, radii, dL/dmeans2D)."""
    from .render import build_cov3D, get_rasterizer
    from .tune import l1_loss, ssim
    g = gaussians
    rast = get_rasterizer(camera, g.active_sh_degree, False, background)
    means2D = torch.zeros_like(g._xyz, requires_grad=True)
    cov = build_cov3D(g.get_scaling, g._rotation, 1.0)
    img, radii = rast(means3D=g._xyz, means2D=means2D, opacities=g.get_opacity, shs=g.get_features, colors_precomp=None,
                      cov3D_precomp=cov)
    gt = gt_image.to(img.device)
    loss = (1.0 - lambda_dssim) * l1_loss(img, gt)
    if lambda_dssim > 0:
        loss = loss + lambda_dssim * (1.0 - ssim(img, gt))
    loss.backward()
    dm2 = means2D.grad
    if step_optimizer:
        g.optimizer.step()
        g.optimizer.zero_grad(set_to_none=True)
        g.invalidate()
    return loss.detach(), radii, dm2


def fit(gaussians, cameras: Sequence, gts: Sequence[Tensor], background: Tensor, opt: SimpleNamespace, extent: float,
        white_background: bool = False, seed: int = 0, native: bool = True, log=None):
    """The training schedule over `opt.iterations` iterations, on the native step (or, native=False, the autograd one: the
    yardstick).  Views come in a seeded random permutation, reshuffled when exhausted.  Returns the loss history."""
    g = gaussians
    rng = random.Random(seed)
    run = NativeGaussianFit(g, background, opt.lambda_dssim, opt.iterations) if native else None
    hist = []
    stack = []
    for it in range(1, int(opt.iterations) + 1):
        g.update_learning_rate(it)
        if it % 1000 == 0:
            g.oneupSHdegree()
        if not stack:
            stack = list(range(len(cameras)))
            rng.shuffle(stack)
        v = stack.pop()
        if native:
            radii, dm2 = run.step(cameras[v], gts[v])
        else:
            loss, radii, dm2 = fit_step_torch(g, cameras[v], gts[v], background, opt.lambda_dssim)
            hist.append(loss)
        if it < opt.densify_until_iter:
            with torch.no_grad():
                vis = radii > 0
                g.max_radii2D = torch.where(vis, torch.max(g.max_radii2D, radii.to(g.max_radii2D.dtype)), g.max_radii2D)
                g.add_densification_stats(dm2, vis)
                if it > opt.densify_from_iter and it % opt.densification_interval == 0:
                    g.densify_and_prune(opt.densify_grad_threshold, 0.005, extent, 20 if it > opt.opacity_reset_interval else None)
                if it % opt.opacity_reset_interval == 0 or (white_background and it == opt.densify_from_iter):
                    g.reset_opacity()
        if log is not None and (it % 1000 == 0 or it == opt.iterations):
            log(f"[{it}/{opt.iterations}] Gaussians {g.get_xyz.shape[0]}")
    return run.losses() if native else torch.stack(hist).double().cpu().numpy() if hist else np.zeros(0)


# ------------------------------------------------------------------ entry point


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fit static 3D Gaussians (kernels.ply) to the views of one time step.")
    p.add_argument("--config", "-c", type=str, required=True, help="finetune-*.yaml or regist-*.yaml (video_data, gaussian.sh_degree)")
    p.add_argument("--output", "-o", type=str, required=True, help="the kernels.ply to write")
    p.add_argument("--frame", type=int, default=None, help="time step to fit (default: the first)")
    p.add_argument("--iterations", type=int, default=DEFAULTS["iterations"])
    p.add_argument("--init_points", type=str, default=None, help="PLY with x, y, z and optional red, green, blue")
    p.add_argument("--init_random", type=int, default=100_000)
    p.add_argument("--init_box", type=float, nargs=6, default=[-1.3, -1.3, -1.3, 1.3, 1.3, 1.3], metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    p.add_argument("--seed", type=int, default=0)
    return p.parse_args(argv)


def initial_cloud(args, rng: np.random.Generator):
    """(points (N,3), colours (N,3) in [0,1]) from --init_points, or --init_random uniform points in --init_box."""
    if args.init_points:
        from .io import read_ply_vertices
        v = read_ply_vertices(args.init_points)
        pts = np.stack((v["x"], v["y"], v["z"]), axis=1).astype(np.float32)
        if all(c in v for c in ("red", "green", "blue")):
            col = np.stack((v["red"], v["green"], v["blue"]), axis=1).astype(np.float32) / 255.0
        else:
            col = np.full_like(pts, 0.5)
        return pts, col
    lo, hi = np.asarray(args.init_box[:3], np.float32), np.asarray(args.init_box[3:], np.float32)
    pts = (lo + (hi - lo) * rng.random((int(args.init_random), 3))).astype(np.float32)
    return pts, rng.random((int(args.init_random), 3)).astype(np.float32)


def reconstruct(cfg, args, log=print) -> int:
    """Returns the number of Gaussians written."""
    from .dataset import VideoDataset
    from .render.gaussian_model import GaussianModel
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    device = torch.device(f"cuda:{cfg.get('gpu', 0)}")
    torch.cuda.set_device(device)
    white = bool(cfg.video_data.data.get("white_background", False))
    background = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    cfg.video_data.device = str(device)
    dataset = VideoDataset(cfg.video_data)
    step = dataset.steps[0] if args.frame is None else args.frame
    cams = [dataset.getCameras(v, step) for v in sorted(dataset.views)]
    gts = [c.original_image.to(device).float().contiguous() for c in cams]
    extent = camera_extent(cams)
    log(f"[reconstruct] {len(cams)} views of step {step}, camera extent {extent:.4f}")
    pts, col = initial_cloud(args, np.random.default_rng(args.seed))
    g = GaussianModel(int(cfg.gaussian.sh_degree)).create_from_pcd(pts, col, extent, device=device)
    opt = fit_options(iterations=int(args.iterations))
    g.training_setup(opt)
    losses = fit(g, cams, gts, background, opt, extent, white_background=white, seed=args.seed, log=log)
    g.save_ply(args.output)
    log(f"[reconstruct] wrote {g.get_xyz.shape[0]} Gaussians to {args.output} (last loss {float(losses[-1]):.6f})")
    return int(g.get_xyz.shape[0])


def main(argv=None):
    from .config import load_config
    args = parse_args(argv)
    reconstruct(load_config(args.config), args)


if __name__ == "__main__":
    sys.exit(main())
