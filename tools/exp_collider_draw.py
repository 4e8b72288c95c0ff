"""Cost of drawing colliders (csrc/nm_draw.hip; DESIGN.md, "Colliders"): the three kernels at 1920x1080 with 8 colliders and
200 000 Gaussians, and the extra cost of one drawn view next to the undrawn one (two more renders plus the three launches).

Kernel times: device events around `reps` back-to-back launches with pre-marshalled arguments, after `warm` launches, repeated
`rounds` times (the median and the spread over the rounds are printed); a launch of a few microseconds is bounded by the launch
rate, which the figure then shows.  View times: device events around whole views, undrawn and drawn alternating.  The cast writes
t, shade and hit: 20 B per pixel, nothing read but its arguments; bytes/s = that over the kernel time.

    python tools/exp_collider_draw.py [reps] [rounds]"""
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from neuma_amd import _lib as L, collider_draw as CD                                # noqa: E402
from neuma_amd.extras import collider_draw as X                                     # noqa: E402
from neuma_amd.sim.colliders import pack, parse_colliders                           # noqa: E402
from neuma_amd.tune import diff_rasterization                                       # noqa: E402
import collider_draw_cases as cc                                                    # noqa: E402

W, H, K = 1920, 1080, 200_000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
warm = 20
assert torch.cuda.is_available(), "needs a GPU (no CPU timing)"
dev = torch.device("cuda", 0)
lib = L.lib()
nodes = cc.SETS["eight"]
colliders, styles = parse_colliders(nodes), CD.parse_styles(nodes)
cam = cc.Camera(W, H, (1.7, 1.25, 2.0), (0.5, 0.45, 0.5), fov_deg=38.0, device=dev)
gen = torch.Generator().manual_seed(0)
means = (torch.tensor([0.5, 0.6, 0.5]) + 0.1 * torch.randn(K, 3, generator=gen)).to(dev).contiguous()
s2 = 0.004 ** 2
cov = torch.tensor([s2, 0.0, 0.0, s2, 0.0, s2]).repeat(K, 1).to(dev).contiguous()
opa = (0.3 + 0.6 * torch.rand(K, 1, generator=gen)).to(dev).contiguous()
shs = torch.rand(K, 16, 3, generator=gen).to(dev).contiguous()
white = torch.ones(3, device=dev)

cfg, inv = CD._cfg(cam), CD._vec(X.inverse_projection(cam).reshape(16), C.c_double)
one, zero, campos = CD._vec((1, 1, 1)), CD._vec((0, 0, 0)), CD._vec(cam.camera_center.cpu())
arr, sty = pack(colliders), CD._styles(styles)
t = torch.empty(H, W, device=dev); shade = torch.empty(3, H, W, device=dev); hit = torch.empty(H, W, dtype=torch.int32, device=dev)
front = torch.empty_like(opa); flags = torch.empty(K, dtype=torch.uint8, device=dev)
img = torch.rand(3, H, W, device=dev); rgb = torch.rand(3, H, W, device=dev); alpha = torch.rand(H, W, device=dev); out = torch.empty(3, H, W, device=dev)
stream = L.stream_ptr(dev)
calls = {
    "k_collider_cast": lambda: lib.nm_collider_cast(C.byref(cfg), inv, one, zero, 8, arr, sty, L.ptr(t), L.ptr(shade), L.ptr(hit), stream),
    "k_collider_hide": lambda: lib.nm_collider_hide(campos, one, zero, 8, arr, K, L.ptr(means), L.ptr(opa), L.ptr(front), L.ptr(flags), stream),
    "k_collider_compose": lambda: lib.nm_collider_compose(C.byref(cfg), L.ptr(img), L.ptr(rgb), L.ptr(alpha), L.ptr(shade), L.ptr(hit),
                                                           L.ptr(out), stream),
}
traffic = {"k_collider_cast": 20 * H * W, "k_collider_hide": (12 + 4 + 4 + 1) * K, "k_collider_compose": (12 + 12 + 4 + 12 + 4 + 12) * H * W}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


print(f"{W}x{H}, 8 colliders, K = {K}; {reps} launches per round, {rounds} rounds, {warm} warm-up launches")
for name, fn in calls.items():
    assert fn() == 0, lib.nm_last_error()
    timed(fn, warm)
    us = [timed(fn, reps) for _ in range(rounds)]
    med = statistics.median(us)
    print(f"  {name:20s} {med:8.2f} us (min {min(us):.2f}, max {max(us):.2f})  {traffic[name] / 1e6:7.2f} MB -> {traffic[name] / med / 1e3:8.1f} GB/s")
print(f"  hit pixels {float((hit >= 0).float().mean()):.3f} of the image, hidden Gaussians {float(flags.float().mean()):.3f}")


def undrawn():
    return diff_rasterization(means, None, None, cam, white, 3, cov, opa, shs)


def drawn():
    return CD.draw(undrawn(), cam, colliders, styles, CD.IDENTITY, CD.front_renderer(means, None, cam, 3, cov, shs), means, opa)


for fn in (undrawn, drawn):
    for _ in range(3):
        fn()
torch.cuda.synchronize()
plain, full = [], []
for _ in range(rounds):
    plain.append(timed(undrawn, 10) / 1e3)
    full.append(timed(drawn, 10) / 1e3)
mp, mf = statistics.median(plain), statistics.median(full)
print(f"  one view undrawn {mp:7.3f} ms (min {min(plain):.3f}, max {max(plain):.3f}); drawn {mf:7.3f} ms (min {min(full):.3f}, max {max(full):.3f}); "
      f"extra {mf - mp:7.3f} ms = {mf / mp:.2f}x")
