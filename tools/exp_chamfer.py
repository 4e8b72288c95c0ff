#!/usr/bin/env python3
"""Chamfer timing (neuma_amd.particle_metrics, python -m neuma_amd.particle_evaluation): one nm_chamfer call (both directions,
indices and means) at N = M = 10^5 with B = 1 and B = 16, and at N = M = 10^6 with B = 1, for two kinds of pairs:
  matched      a jittered lattice ball (the synth.py particle layout) against a smoothly deformed copy of itself: prediction
               against ground truth of one object, the use of particle_evaluation
  ball_cube    the same ball against a uniform cube around it: about half of the cube's points lie outside the ball, in empty
               cells of its grid, and walk many shells (the slow case of the grid search)
and, for context, scipy cKDTree on the host at the same sizes (build + query, both directions, one batch item).

    python tools/exp_chamfer.py [--iters 20] [--warmup 3] [--no-kdtree] [--cases matched,ball_cube]

prints one JSON line: ms per call (CUDA events around --iters back-to-back calls) and ms of cKDTree per item.
Per-kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o chamfer -- python tools/exp_chamfer.py --no-kdtree
(k_nn_box, k_nn_grid, k_nn_count, k_nn_scatter, k_nn_search, k_nn_mean_part, k_nn_mean_finish and rocPRIM's scan)."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests" / "golden"))

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


def clouds(kind, B, n, seed=0):
    import chamfer_inputs as CI
    r = np.random.Generator(np.random.PCG64(seed))
    base = CI._lattice_ball(n, max(16, int(round((n / 8) ** (1 / 3)))), r)
    a = np.stack([base + r.normal(0, 1e-3, base.shape) for _ in range(B)]).astype(np.float32)
    if kind == "matched":
        b = a + 0.03 * np.sin(2 * np.pi * a[..., [1, 2, 0]]) + r.normal(0, 2e-3, a.shape)
    else:
        b = r.uniform(0.2, 0.8, (B, n, 3)) + 0.01 * r.normal(size=(B, n, 3))
    return a, b.astype(np.float32)


def kdtree_ms(a, b):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    cKDTree(b.astype(np.float64)).query(a.astype(np.float64), k=1)
    cKDTree(a.astype(np.float64)).query(b.astype(np.float64), k=1)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--cases", default="matched,ball_cube")
    args = ap.parse_args()
    from neuma_amd.particle_metrics import chamfer_native
    dev = torch.device("cuda", 0)
    out = {}
    for kind in args.cases.split(","):
        for B, n in ((1, 100_000), (16, 100_000), (1, 1_000_000)):
            a, b = clouds(kind, B, n)
            ga, gb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            key = f"{kind}_B{B}_N{n}"
            out[f"chamfer_ms_{key}"] = round(time_calls(lambda: chamfer_native(ga, gb), args.iters, args.warmup), 4)
            if not args.no_kdtree:
                out[f"ckdtree_ms_per_item_{key}"] = round(kdtree_ms(a[0], b[0]), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
