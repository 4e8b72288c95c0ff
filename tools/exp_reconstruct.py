#!/usr/bin/env python3
"""Times of the static Gaussian fit on one GPU: NativeGaussianFit.step beside fit_step_torch (2000 Gaussians, 96 x 96, and
K = 200 000 at 480 x 270), nm_knn_mean_dist2 at 10^5 and 10^6 points, and the two activation launches at K = 200 000.
Prints one JSON line per figure (median of `--reps` timed runs after `--warmup`)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def model(K, d, seed=0):
    from neuma_amd.reconstruct import fit_options
    from neuma_amd.render.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    m = GaussianModel(1)
    m.set_params(*(t.float().to(d) for t in (0.25 + 0.5 * torch.rand(K, 3, generator=g), torch.randn(K, 1, 3, generator=g),
                                             0.2 * torch.randn(K, 3, 3, generator=g), torch.log(0.004 + 0.01 * torch.rand(K, 3, generator=g)),
                                             torch.randn(K, 4, generator=g), torch.randn(K, 1, generator=g))))
    m.spatial_lr_scale = 1.0
    m.training_setup(fit_options())
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from neuma_amd import synth
    from neuma_amd.reconstruct import NativeGaussianFit, fit_step_torch
    from neuma_amd.render import gaussian_activate, gaussian_activate_backward
    from neuma_amd.render.simple_knn import distCUDA2
    d = torch.device("cuda", 0)
    bg = torch.zeros(3, device=d)
    for K, W, H in ((2000, 96, 96), (200_000, 480, 270)):
        cam = synth.ring_cameras(1, W, H, device=d)[0]
        gt = torch.rand(3, H, W, device=d)
        m = model(K, d)
        run = NativeGaussianFit(m, bg, 0.2, a.warmup + a.reps)
        print(json.dumps({"what": "NativeGaussianFit.step", "K": K, "W": W, "H": H, "ms": timed(lambda: run.step(cam, gt), a.warmup, a.reps)}))
        m = model(K, d)
        print(json.dumps({"what": "fit_step_torch", "K": K, "W": W, "H": H,
                          "ms": timed(lambda: fit_step_torch(m, cam, gt, bg, 0.2), a.warmup, a.reps)}))
    for n in (100_000, 1_000_000):
        pts = torch.rand(n, 3, device=d)
        print(json.dumps({"what": "nm_knn_mean_dist2 k=3", "n": n, "ms": timed(lambda: distCUDA2(pts), a.warmup, a.reps)}))
    m = model(200_000, d)
    ls, rot, op = m._scaling.detach(), m._rotation.detach(), m._opacity.detach()
    gc, go = torch.randn(200_000, 6, device=d), torch.randn(200_000, 1, device=d)
    print(json.dumps({"what": "nm_gaussian_activate", "K": 200_000, "ms": timed(lambda: gaussian_activate(ls, rot, op), a.warmup, a.reps)}))
    print(json.dumps({"what": "nm_gaussian_activate_backward", "K": 200_000,
                      "ms": timed(lambda: gaussian_activate_backward(ls, rot, op, 1.0, gc, go), a.warmup, a.reps)}))


if __name__ == "__main__":
    main()
