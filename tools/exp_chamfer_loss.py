#!/usr/bin/env python3
"""Chamfer loss timing: the native chamfer_loss (nm_chamfer_loss: forward + backward, the gradient comes out of the forward
launch) against the composition particle_metrics.chamfer_distance_kdtree + .backward() (nm_chamfer, then torch gather /
scatter_add_), at N = M = 100 000: x uniform in a ball, y = x[perm] + 1 % noise.

    python tools/exp_chamfer_loss.py [--n 100000] [--repeats 5] [--calls 200] [--warmup 10] [--epoch]

The two alternate inside one run, after warm-up: per repeat, --calls calls of one, then --calls calls of the other, host clock
around a synchronised window.  These are CALL times (launches, allocations and the Python around them included), not kernel
times; per-kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o chamfer_loss -- python tools/exp_chamfer_loss.py --repeats 1 --calls 20
--epoch adds one pretraining epoch (3 frames x 10 substeps, the body of tests/pretrain_cases.py) with the state loss and with the
Chamfer loss.  Prints one JSON line: median and min..max ms per call, and the bytes a call needs from the shapes."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def epoch_times(repeats):
    import pretrain_cases as pc
    from neuma_amd.pretrain import FrameStepper, chamfer_frame_loss, epoch_loss, generate_trajectory
    from neuma_amd.state_loss import state_loss
    model, st, init = pc.body()
    with torch.no_grad():
        traj = generate_trajectory(model, st, init, *pc.neural_pair("jelly"), pc.T, pc.S)
    E, P = pc.neural_pair("jelly", final_scale=0.8)
    sim = FrameStepper(model, st, E, P, pc.S, pc.T)
    ws = [p for p in list(E.parameters()) + list(P.parameters()) if p.requires_grad]

    def epoch(fn):
        loss, _ = epoch_loss(sim, traj, pc.T, loss_fn=fn, start=init)
        torch.autograd.grad(loss, ws)

    out = {"state": [], "chamfer": []}
    fns = {"state": state_loss, "chamfer": chamfer_frame_loss(1.0, 1.0)}
    for fn in fns.values():
        epoch(fn)
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(lambda: epoch(fn), 5))
    return {f"epoch_ms_{k}": stats(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--epoch", action="store_true")
    args = ap.parse_args()
    from neuma_amd import _lib
    from neuma_amd.chamfer_loss import chamfer_loss
    from neuma_amd.particle_metrics import chamfer_distance_kdtree
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    n = args.n
    p = rng.standard_normal((n, 3))
    p *= (rng.random((n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(p, axis=1, keepdims=True)
    x = (0.5 + 0.3 * p).astype(np.float32)                                          # uniform in a ball of radius 0.3
    y = (x[rng.permutation(n)] + 0.01 * 0.3 * rng.standard_normal((n, 3))).astype(np.float32)
    tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev)

    def native():
        tx.grad = None
        chamfer_loss(tx, ty).backward()

    def composed():
        tx.grad = None
        chamfer_distance_kdtree(tx[None], ty[None]).sum().backward()

    for fn in (native, composed):
        for _ in range(args.warmup):
            fn()
    t = {"native": [], "composition": []}
    for _ in range(args.repeats):
        t["native"].append(window(native, args.calls))
        t["composition"].append(window(composed, args.calls))
    m = n
    out = {"n": n, "m": m, "calls": args.calls, "repeats": args.repeats,
           "call_ms_native": stats(t["native"]), "call_ms_composition": stats(t["composition"]),
           # what one call must move at least: x, y read by the binning and again as sorted float4 by both searches, the indices
           # and distances written, the (b, j) pairs sorted (a 32-bit key and value in, out), the gradient written
           "bytes_inputs": 12 * (n + m), "bytes_gradient": 12 * n,
           "bytes_algorithmic": 12 * (n + m) + 2 * 16 * (n + m) + 16 * (n + m) + 16 * m + 12 * m + 12 * n,
           "workspace_bytes": int(_lib.lib().nm_chamfer_loss_workspace(n, m))}
    if args.epoch:
        out.update(epoch_times(args.repeats))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
