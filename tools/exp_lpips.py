#!/usr/bin/env python3
"""LPIPS timing (python -m neuma_amd.evaluation --lpips_vgg ... --lpips_heads ...): nm_lpips on 11 pairs of 3x360x360 (the
evaluation's default: 11 cropped frames) with seeded random weights, next to the same chain through torch's own fp32
`F.conv2d` / `F.max_pool2d` on the same card, and each convolution layer of the native chain on its own.

    python tools/exp_lpips.py [--iters 40] [--warmup 3] [--pairs 11] [--size 360]

prints one JSON line: ms per call (HIP events around --iters back-to-back calls; native and torch alternate over three rounds,
the median round is reported and all rounds are listed), the achieved TFLOP/s of the convolutions
(2 * 9 * Cin * Cout * H * W per layer and image; the heads, pools and the scale step are not counted as work) next to the
157.3 TFLOP/s f32-matrix peak, and the per-layer figures."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3


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


def layer_shapes(h, w):
    """(cin, cout, h, w) of the 13 convolutions for an h x w image"""
    from neuma_amd.extras import lpips as twin
    out = []
    for i, (ci, co) in enumerate(twin.CONV_CHANNELS):
        out.append((ci, co, h, w))
        if i in twin.POOL_AFTER:
            h, w = h // 2, w // 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=11)
    ap.add_argument("--size", type=int, default=360)
    args = ap.parse_args()
    from neuma_amd import lpips as nl
    from neuma_amd.extras import lpips as twin
    dev = torch.device("cuda", 0)
    convs, heads = twin.random_weights(7)
    W = nl.LpipsWeights(convs, heads, dev)
    g = torch.Generator().manual_seed(0)
    shape = (args.pairs, 3, args.size, args.size)
    a = torch.rand(shape, generator=g)
    b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    a, b = a.to(dev), b.to(dev)
    shapes = layer_shapes(args.size, args.size)
    flop = 2 * args.pairs * sum(2 * 9 * ci * co * h * w for ci, co, h, w in shapes)
    out = {"pairs": args.pairs, "size": args.size, "conv_GFLOP": round(flop / 1e9, 1), "peak_f32_matrix_TFLOPs": PEAK_F32_MATRIX_TFLOPS}

    cw = [(w.to(dev), bb.to(dev)) for w, bb in convs]
    hw = [h.to(dev) for h in heads]

    def torch_chain():
        with torch.no_grad():
            return twin.lpips(a, b, cw, hw, dtype=torch.float32)

    big = 1 << 33       # one nm_lpips call for all pairs
    rounds = {"one_call": [], "default": [], "torch": []}
    for _ in range(3):
        rounds["one_call"].append(time_calls(lambda: nl.lpips(a, b, W, workspace_budget=big), args.iters, args.warmup))
        rounds["torch"].append(time_calls(torch_chain, args.iters, args.warmup))
        rounds["default"].append(time_calls(lambda: nl.lpips(a, b, W), args.iters, args.warmup))
    ms_one, ms_def, ms_t = (sorted(rounds[k])[1] for k in ("one_call", "default", "torch"))
    tf = lambda ms: round(flop / (ms * 1e-3) / 1e12, 2)      # noqa: E731
    out["native"] = {"ms_one_call": round(ms_one, 3), "TFLOPs_one_call": tf(ms_one), "ms_default_1GiB_chunks": round(ms_def, 3),
                     "TFLOPs_default": tf(ms_def)}
    out["torch_fp32_conv2d"] = {"ms": round(ms_t, 3), "TFLOPs": tf(ms_t)}
    out["rounds_ms"] = {k: [round(v, 3) for v in vs] for k, vs in rounds.items()}
    v_native = nl.lpips(a, b, W).cpu()
    v_torch = torch_chain().cpu()
    out["max_rel_native_vs_torch_fp32"] = float(((v_native - v_torch).abs() / v_torch).max())

    layers = []
    n = 2 * args.pairs
    for (ci, co, h, w), (wp, bias) in zip(shapes, W.packed):
        x = torch.relu(torch.randn(n, h, w, ci, device=dev))
        ms = time_calls(lambda: nl.conv3x3_relu(x, wp, bias), 5 * args.iters, args.warmup)
        f = n * 2 * 9 * ci * co * h * w
        layers.append({"cin": ci, "cout": co, "hw": [h, w], "ms": round(ms, 3), "TFLOPs": round(f / (ms * 1e-3) / 1e12, 2)})
        del x
    out["native_layers"] = layers
    print(json.dumps(out))


if __name__ == "__main__":
    main()
