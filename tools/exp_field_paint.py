"""Cost of the field-paint kernels next to the binding product of the same frame: 100 000 particles, 200 000 Gaussians with 8 bound
particles each, every launch timed with nm_prof_enable(1).  Prints mean microseconds per launch of k_particle_field (per quantity),
k_field_paint in its three forms (row walk to g only; row walk and colour; colour of given values), the two k_field_range kernels,
and k_spmm_csr as compute_bindings_F launches it (9 columns) - the yardstick ("Field paint").
    python tools/exp_field_paint.py [iterations]"""
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from neuma_amd import _lib as L, field_paint as fp                                  # noqa: E402
from neuma_amd.tune import Bindings, compute_bindings_F                             # noqa: E402

N, K, NB = 100_000, 200_000, 8
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(0)
# every Gaussian binds NB particles near its own index, as a spatially sorted cloud does
rows = torch.arange(K).repeat_interleave(NB)
cols = ((torch.arange(K) * N // K).repeat_interleave(NB) + torch.randint(-200, 200, (K * NB,), generator=gen)).clamp(0, N - 1)
b = Bindings(torch.stack([rows, cols]), torch.rand(K * NB, generator=gen) + 0.05, (K, N), dev)
x0 = torch.rand(N, 3, generator=gen).to(dev)
x = x0 + 0.01
v = torch.randn(N, 3, generator=gen).to(dev)
F = (torch.eye(3) + 0.1 * torch.randn(N, 3, 3, generator=gen)).to(dev)
S = (50.0 * torch.randn(N, 3, 3, generator=gen)).to(dev)
lib = L.lib()


def timed(label, fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    lib.nm_prof_reset(); lib.nm_prof_enable(1, None)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    lib.nm_prof_enable(0, None)
    buf = C.create_string_buffer(1 << 16)
    lib.nm_prof_report(buf, len(buf))
    for r in buf.value.decode().splitlines():
        if r.strip():
            name, count, total = r.split()[0], int(r.split()[1]), float(r.split()[2])
            print(f"  {label:34s} {name:24s} {count:5d} launches  {1e3 * total / count:8.2f} us each")


print(f"N={N} particles, K={K} Gaussians, {NB} bound particles each, {iters} iterations")
timed("compute_bindings_F (yardstick)", lambda: compute_bindings_F(F, b))
given = dict(x=x, v=v, F=F, stress=S, x0=x0)
q = None
for name in fp.QUANTITIES:
    timed(f"particle_field {name}", lambda: fp.particle_field(name, **{k: given[k] for k in fp.NEEDS[name]}))
q = fp.particle_field("von_mises", F=F, stress=S)
rng = torch.tensor([0.0, 100.0], device=dev)
timed("paint: row walk, g only", lambda: fp.paint_raw(q, b, want_dc=False))
timed("paint: row walk and colour", lambda: fp.paint_raw(q, b, "heat", rng))
g = fp.paint_raw(q, b, want_dc=False)[1]
timed("paint: colour of given g", lambda: fp.paint_raw(g, None, "heat", rng, want_g=False))
timed("range of g", lambda: fp.field_range(g))
painter = fp.FieldPainter("von_mises")
timed("painter.frame, automatic range", lambda: painter.frame(x, v, F, lambda F_: S, b))
