#!/usr/bin/env python3
"""Image-metric timing (python -m neuma_amd.evaluation): one nm_image_metrics call (PSNR sums + SSIM, per-image ranges) on
B = 11 x 3x360x360 (the evaluation's default: 11 cropped frames) and B = 16 x 3x1080x1920, and, for scale, the host side of the
entry point on 11 800x800 frames (PNG decode of prediction + ground truth, compositing, crop).

    python tools/exp_image_metrics.py [--iters 50] [--warmup 5]

prints one JSON line: ms per call of each batch (CUDA events around --iters back-to-back calls) and ms of the host side.
Per-launch kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o metrics -- python tools/exp_image_metrics.py
(k_metrics_stats, k_metrics_range, k_metrics_ssim, k_metrics_finish in the stats CSV)."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def time_calls(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def host_side_ms(n=11, size=800):
    from PIL import Image
    from neuma_amd import evaluation as ev
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8), "RGB").save(f"{d}/p{i}.png")
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(f"{d}/g{i}.png")
        t0 = time.perf_counter()
        for i in range(n):
            ev.crop(ev.load_pred(f"{d}/p{i}.png"))
            ev.crop(ev.load_gt(f"{d}/g{i}.png"))
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from neuma_amd.image_metrics import image_metrics
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {}
    for tag, shape in (("11x3x360x360", (11, 3, 360, 360)), ("16x3x1080x1920", (16, 3, 1080, 1920))):
        p = torch.rand(shape, generator=g).to(dev)
        t = (p + 0.05 * torch.randn(shape, generator=g).to(dev)).clamp(0, 1)
        ms = time_calls(lambda: image_metrics(p, t), args.iters, args.warmup)
        gb = 2 * p.numel() * 4 * 2 / 1e9          # both inputs read by each pass
        out[tag] = {"ms_per_call": round(ms, 4), "GB_per_s_two_passes": round(gb / (ms * 1e-3), 1)}
        del p, t
    out["host_decode_11x800x800_ms"] = round(host_side_ms(), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
