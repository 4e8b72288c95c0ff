"""Cost of drawing mesh colliders (csrc/nm_draw.hip k_field_cast / k_field_hide; DESIGN.md, "Drawing mesh colliders"): the two
kernels at 1920x1080 with the four mesh colliders of tools/exp_mesh_sdf.py (resolution 64) and 200 000 Gaussians, next to
k_collider_cast with the 8 analytic colliders of tools/exp_collider_draw.py in the same run (the yardstick); the mean number of
march steps per hit pixel (from the fp64 definition on a 240x135 image of the same view); and one drawn view next to the undrawn one.

Kernel times: device events around `reps` back-to-back launches with pre-marshalled arguments, after `warm` launches, repeated
`rounds` times (the median and the spread over the rounds are printed).  Every k_field_cast launch starts from the same buffers
(+inf / 0 / -1: an empty analytic cast), restored by three device copies inside the timed region; the copies alone are timed too
and subtracted.  View times: device events around whole views, undrawn and drawn alternating.

    python tools/exp_mesh_draw.py [reps] [rounds]"""
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from neuma_amd import _lib as L, collider_draw as CD                                # noqa: E402
from neuma_amd.extras import collider_draw as X, mesh_draw as XM                    # noqa: E402
from neuma_amd.sim.colliders import pack, pack_fields, parse_colliders              # noqa: E402
from neuma_amd.tune import diff_rasterization                                       # noqa: E402
import collider_draw_cases as cc                                                    # noqa: E402
import mesh_sdf_cases as cases                                                      # noqa: E402

W, H, K = 1920, 1080, 200_000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
warm = 10
assert torch.cuda.is_available(), "needs a GPU (no CPU timing)"
dev = torch.device("cuda", 0)
lib = L.lib()
meshes = [("torus", "friction"), ("box", "slip"), ("sphere320", "sticky"), ("icosahedron", "friction")]
nodes = [dict(type="mesh", verts=cases.MESHES[m]()[0], tris=cases.MESHES[m]()[1], resolution=64, surface=s,
              friction=0.4 if s == "friction" else 0.0, velocity=[0, 0.1 * i, 0]) for i, (m, s) in enumerate(meshes)]
fields = [c.build(dev) for c in parse_colliders(nodes)]
fstyles = CD.parse_mesh_styles(nodes, 0)
anodes = cc.SETS["eight"]
colliders, styles = parse_colliders(anodes), CD.parse_styles(anodes)
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
farr, fsty = pack_fields(fields), CD._styles(fstyles)
t = torch.empty(H, W, device=dev); shade = torch.empty(3, H, W, device=dev); hit = torch.empty(H, W, dtype=torch.int32, device=dev)
t0 = torch.full((H, W), float("inf"), device=dev); shade0 = torch.zeros(3, H, W, device=dev)
hit0 = torch.full((H, W), -1, dtype=torch.int32, device=dev)
front = opa.clone(); flags = torch.zeros(K, dtype=torch.uint8, device=dev)
stream = L.stream_ptr(dev)


def restore():
    t.copy_(t0); shade.copy_(shade0); hit.copy_(hit0)
    return 0


def field_cast():
    restore()
    return lib.nm_collider_cast_field(C.byref(cfg), inv, one, zero, len(fields), farr, fsty, 0, L.ptr(t), L.ptr(shade), L.ptr(hit), stream)


calls = {
    "k_collider_cast (8 analytic)": lambda: lib.nm_collider_cast(C.byref(cfg), inv, one, zero, 8, arr, sty, L.ptr(t), L.ptr(shade), L.ptr(hit), stream),
    "restore (3 copies)": restore,
    "k_field_cast + restore": field_cast,
    "k_field_hide": lambda: lib.nm_collider_hide_field(campos, one, zero, len(fields), farr, K, L.ptr(means), L.ptr(front), L.ptr(flags), stream),
}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def measure(name, fn):
    assert fn() == 0, lib.nm_last_error()
    timed(fn, warm)
    us = [timed(fn, reps) for _ in range(rounds)]
    print(f"  {name:34s} {statistics.median(us):9.2f} us (min {min(us):.2f}, max {max(us):.2f})")
    return statistics.median(us)


print(f"{W}x{H}, {len(fields)} mesh colliders" + "".join(f", lattice {'x'.join(map(str, c.dims))}" for c in fields)
      + f", K = {K}; {reps} launches per round, {rounds} rounds, {warm} warm-up launches")
res = {}
for name in ("k_collider_cast (8 analytic)", "restore (3 copies)", "k_field_hide"):
    res[name] = measure(name, calls[name])
m = measure("k_field_cast + restore", field_cast)
print(f"  {'k_field_cast':34s} {m - res['restore (3 copies)']:9.2f} us (restore subtracted)")
print(f"  hit pixels {float((hit >= 0).float().mean()):.3f} of the image, hidden Gaussians {float(flags.float().mean()):.3f}")

# the mean number of march steps: the fp64 definition on a small image of the same view
small = cc.Camera(240, 135, (1.7, 1.25, 2.0), (0.5, 0.45, 0.5), fov_deg=38.0)
base = X.cast(small, [], [], X.IDENTITY)
_, _, shit, _, steps = XM.cast_field(small, fields, fstyles, X.IDENTITY, *base, margins=True)
print(f"  march steps per hit pixel (240x135, fp64 definition, the winning field's march): mean {float(steps[shit >= 0].float().mean()):.1f}, "
      f"max {int(steps.max())}; hit pixels {float((shit >= 0).float().mean()):.3f}")


def undrawn():
    return diff_rasterization(means, None, None, cam, white, 3, cov, opa, shs)


def drawn():
    return CD.draw(undrawn(), cam, [], [], CD.IDENTITY, CD.front_renderer(means, None, cam, 3, cov, shs), means, opa,
                   fields=fields, field_styles=fstyles)


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
