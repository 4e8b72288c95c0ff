#!/usr/bin/env python3
"""Time of one nm_gaussian_deform launch at the metric workload's K = 200 000 Gaussians on one GPU, beside the nm_gaussian_activate
launch it sits next to: device events around windows of `--calls` back-to-back launches into preallocated outputs (so the figure is
the launch, not the allocator), `--windows` windows after `--warmup` launches.  Prints one JSON line per kernel: median, min and max
of the per-call time over the windows, and the 92 B (52 B) per Gaussian over the median."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def windows(fn, warmup, n_windows, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)          # us per call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--calls", type=int, default=500)
    a = ap.parse_args()
    from neuma_amd import _lib as L
    d = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    K = a.K
    ls = torch.log(0.001 + 0.099 * torch.rand(K, 3, generator=g)).to(d)
    rot = torch.randn(K, 4, generator=g).to(d)
    F = (torch.eye(3)[None] + 0.3 * torch.randn(K, 3, 3, generator=g)).to(d)
    lo, q, cov6 = torch.empty(K, 3, device=d), torch.empty(K, 4, device=d), torch.empty(K, 6, device=d)
    lib, st = L.lib(), L.stream_ptr(d)
    deform = lambda: L.check(lib.nm_gaussian_deform(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(q), st))
    activate = lambda: L.check(lib.nm_gaussian_activate(K, L.ptr(ls), L.ptr(rot), None, 1.0, L.ptr(cov6), None, st))
    for what, fn, nbytes in (("nm_gaussian_deform", deform, 92), ("nm_gaussian_activate (cov6 only)", activate, 52)):
        t = windows(fn, a.warmup, a.windows, a.calls)
        med = statistics.median(t)
        print(json.dumps({"what": what, "K": K, "us_per_call_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                          "windows": a.windows, "calls_per_window": a.calls, "bytes_per_gaussian": nbytes,
                          "GB_per_s_at_median": round(nbytes * K / med * 1e-3, 1)}))


if __name__ == "__main__":
    main()
