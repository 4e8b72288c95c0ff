#!/usr/bin/env python3
"""Registration loop timing (python -m neuma_amd.regist): the native iteration (nm_regist_apply, 3 x render forward + pixel loss
+ nm_ssim_loss + render adjoint + nm_regist_backward, RAdam on 10 scalars) against the torch autograd path (Register.forward +
build_cov3D + GaussianRasterizer + tune.ssim) on a synthetic scene of the `burger` configuration (200k Gaussians, 3 views,
1920x1080, sh 0) from synth.py, ground truth rendered at a known transform.  --sh DEG: the same scene with SH colours of that
degree, rotated with the Gaussians every iteration (nm_sh_rotate / nm_sh_rotate_backward; the targets too).

    python tools/exp_regist.py [--iters 200] [--warmup 20] [--lam 0.1] [--mask] [--only native|torch] [--sh 0..3]

prints one JSON line: iterations/s of both paths.  Per-launch kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o regist -- python tools/exp_regist.py --only native --iters 50
(k_regist_apply, k_regist_bwd + k_regist_reduce, k_ssim_fwd + k_ssim_bwd, with --sh 1..3 k_sh_rotate, k_sh_rotate_bwd +
k_sh_rotate_finish in the stats CSV)."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def scene(dev, K, W, H, V, sh=0):
    from neuma_amd import synth
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = synth.make_scene("burger", override=dict(K=K, W=W, H=H, V=V, sh=sh))
    gm = GaussianModel(sc.cfg["sh"])
    sh = torch.tensor(sc.g_sh, device=dev)
    gm.set_params(torch.tensor(sc.g_xyz, device=dev), sh[:, :1].contiguous(), sh[:, 1:].contiguous(), torch.tensor(sc.g_logscale, device=dev),
                  torch.tensor(sc.g_rot, device=dev), torch.tensor(sc.g_opacity_logit, device=dev))
    return gm, synth.ring_cameras(V, W, H, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--mask", action="store_true")
    ap.add_argument("--only", choices=["native", "torch"], default=None)
    ap.add_argument("--K", type=int, default=200_000)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--V", type=int, default=3)
    ap.add_argument("--sh", type=int, default=0, choices=[0, 1, 2, 3], help="SH degree of the scene's colours")
    a = ap.parse_args()
    from neuma_amd.regist import NativeRegistration, Register, euler_to_quat, pack_params, quat_to_rot6d, regist_apply, regist_step_torch
    from neuma_amd.render import flush_pending, raster_forward_raw
    dev = torch.device("cuda", 0)
    gm, cams = scene(dev, a.K, a.W, a.H, a.V, a.sh)
    bg = torch.zeros(3, device=dev)
    sched = dict(max_steps=20000, learning_rate_alpha=0.01)
    cfg = dict(INIT_R=[0.0, 0.0, 0.0], INIT_T=[0.0, 0.0, 0.0], INIT_S=[1.0], lr_r=1e-4, lr_t=5e-5, lr_s=1e-5, scheduler=sched)
    # ground truth at a known transform (3 degrees, 1 % translation, 2 % scale)
    truth = Register(dict(cfg, INIT_R=[3.0, -2.0, 1.0], INIT_T=[0.005, -0.004, 0.003], INIT_S=[1.02]), device=dev)
    probe = NativeRegistration(truth, gm, cams, [torch.zeros(3, a.H, a.W, device=dev)] * a.V, bg, force_mask_data=a.mask)
    with torch.no_grad():
        _, _, params = pack_params(truth, probe.origin)
        m, c6 = regist_apply(probe.xyz, probe.ls, probe.rot, params)
        sh = probe._rotated_sh(params) if probe.rotate_sh else probe.sh
        gts = [raster_forward_raw(cam, m, sh, probe.cp, probe.op, c6)[0].clone() for cam in probe.cams]
    flush_pending()
    out = {"K": a.K, "W": a.W, "H": a.H, "views": a.V, "lambda_ssim": a.lam, "mask": a.mask, "iters": a.iters, "sh": a.sh}
    if a.only in (None, "native"):
        reg = Register(cfg, device=dev)
        reg.training_setup()
        run = NativeRegistration(reg, gm, cams, gts, bg, lambda_ssim=a.lam, force_mask_data=a.mask, num_iter=a.warmup + a.iters)
        for _ in range(a.warmup):
            run.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            run.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        flush_pending()
        h = run.losses()
        out.update(native_it_s=a.iters / dt, native_ms_per_iter=1e3 * dt / a.iters, native_loss_first=float(h[0]), native_loss_last=float(h[-1]))
    if a.only in (None, "torch"):
        reg = Register(cfg, device=dev)
        reg.training_setup()
        for _ in range(a.warmup):
            loss, _ = regist_step_torch(reg, gm, cams, gts, bg, lambda_ssim=a.lam, force_mask_data=a.mask)
            float(loss)                                                   # the reference's loss.item() per iteration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            loss, _ = regist_step_torch(reg, gm, cams, gts, bg, lambda_ssim=a.lam, force_mask_data=a.mask)
            float(loss)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        flush_pending()
        out.update(torch_it_s=a.iters / dt, torch_ms_per_iter=1e3 * dt / a.iters)
    if "native_it_s" in out and "torch_it_s" in out:
        out["speedup"] = out["native_it_s"] / out["torch_it_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
