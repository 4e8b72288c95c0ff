#!/usr/bin/env python3
"""Pretraining timings at the `sf` particle count (100 000 particles, grid 128, dt 5e-4, the `sand` base model):

  loss   one frame's state loss with both gradients: state_loss (nm_state_loss: k_state_loss + k_state_finish, + k_state_count
         with a mask) against state_loss_torch (F.mse_loss twice + autograd), forward + backward, l2, with velocities;
  epoch  one pretraining epoch (--frames frames of --substeps fused substeps, loss after every frame, one backward()) with
         each of the two losses.

    python tools/exp_pretrain.py [--n 100000] [--iters 200] [--warmup 20] [--repeats 5] [--frames 3] [--substeps 10] [--mask]

The two versions alternate inside every repeat; each window ends in a device synchronise; the JSON line carries the median and
the min / max over the repeats (the spread) of both, and the algorithmic bytes of the loss (x, v, x_gt, v_gt read, two
gradients written: 72 B per particle, + 2 B with a mask, which the count pass reads once more).  Kernel times come from a
run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o pretrain -- python tools/exp_pretrain.py --only loss --repeats 1
Needs a GPU: without one it fails (a CPU timing says nothing about the MI355X)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def compare(fns, iters, warmup, repeats):
    """{name: (median, min, max) us per call}; the versions alternate inside every repeat"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=10)
    ap.add_argument("--epoch_iters", type=int, default=5)
    ap.add_argument("--mask", action="store_true")
    ap.add_argument("--only", choices=["loss", "epoch"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "exp_pretrain.py measures on the GPU"
    from neuma_amd import synth
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    from neuma_amd.pretrain import FrameStepper, epoch_loss, generate_trajectory
    from neuma_amd.sim import MPMModelBuilder
    from neuma_amd.state_loss import state_loss, state_loss_torch
    dev = torch.device("cuda", 0)
    G = 128
    x0 = torch.tensor(synth.ball_particles(a.n, G), device=dev)
    n = x0.shape[0]
    out = dict(n=n, mask=a.mask, iters=a.iters, repeats=a.repeats, loss_bytes=n * (72 + (2 if a.mask else 0)))
    g = torch.Generator(device=dev).manual_seed(0)
    mask = (torch.rand(n, device=dev, generator=g) < 0.7).to(torch.uint8) if a.mask else None
    if a.only in (None, "loss"):
        x, v = (torch.rand(n, 3, device=dev, generator=g).requires_grad_(True) for _ in range(2))
        xg, vg = (torch.rand(n, 3, device=dev, generator=g) for _ in range(2))

        def run(fn):
            def one():
                x.grad = v.grad = None
                fn(x, v, xg, vg, mask).backward()
            return one

        out["loss"] = compare(dict(native=run(state_loss), torch=run(state_loss_torch)), a.iters, a.warmup, a.repeats)
        out["loss"]["native_GBps_algorithmic"] = out["loss_bytes"] / out["loss"]["native"]["median_us"] * 1e-3
    if a.only in (None, "epoch"):
        model = MPMModelBuilder().parse_cfg(dict(gravity=[0.0, -9.8, 0.0], bc="noslip", num_grids=G, dt=5e-4, bound=1, eps=6e-7)).finalize(dev, True)
        st = model.statics(n)
        st.vol.fill_((0.5 / G) ** 3); st.rho.fill_(1000.0); st.clip_bound.fill_(0.1); st.enabled.fill_(1)
        cfg = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)
        w = synth.load_base_weights("sand")

        def pair(scale):
            E, P = InvariantFullMetaElasticity(cfg), InvariantFullMetaPlasticity(cfg)
            for net, tag in ((E, "e"), (P, "p")):
                for lin, arr in zip((net.layers[0].fc, net.layers[1].fc, net.final_layer.fc), w[tag]):
                    lin.weight.data.copy_(torch.tensor(arr))
                net.final_layer.fc.weight.data.mul_(scale)
                net.to(dev)
            return E, P

        F0 = torch.diag(torch.tensor([1.1, 0.92, 1.0])).to(dev).repeat(n, 1, 1).contiguous()
        init = (x0, torch.tensor([0.0, -0.5, 0.0], device=dev).repeat(n, 1), torch.zeros(n, 3, 3, device=dev), F0)
        traj = generate_trajectory(model, st, init, *pair(1.0), a.frames, a.substeps)
        traj.mask = mask
        E, P = pair(0.8)
        sim = FrameStepper(model, st, E, P, a.substeps, a.frames, fused="true")
        ws = list(E.parameters()) + list(P.parameters())

        def run(fn):
            def one():
                for p in ws:
                    p.grad = None
                epoch_loss(sim, traj, a.frames, loss_fn=fn)[0].backward()
            return one

        out["epoch"] = compare(dict(native=run(state_loss), torch=run(state_loss_torch)), a.epoch_iters, 2, a.repeats)
        out["epoch"].update(frames=a.frames, substeps=a.substeps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
