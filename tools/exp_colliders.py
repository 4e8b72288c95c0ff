"""Cost of the collider kernels next to the grid update they follow: 100 000 particles on the 128^3 grid, 8 colliders that all
cut the body (3 planes, 3 spheres, 2 boxes; every surface kind), one differentiable substep per iteration, every launch timed
with nm_prof_enable(1).  Prints mean microseconds per launch of k_grid_op / k_grid_collide / k_grid_op_bwd / k_grid_collide_bwd
("Colliders").   python tools/exp_colliders.py [iterations]"""
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from neuma_amd import _lib as L                                                     # noqa: E402
from neuma_amd.sim import MPMDiffSim, MPMModelBuilder                               # noqa: E402

N, G = 100_000, 128
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(0)
x = 0.3 + 0.4 * torch.rand(N, 3, generator=gen)
cell = torch.floor(x * G).long()
x = x[torch.argsort((cell[:, 0] * G + cell[:, 1]) * G + cell[:, 2])].contiguous()
v = torch.randn(N, 3, generator=gen)
Cm = torch.zeros(N, 3, 3)
F = torch.eye(3).repeat(N, 1, 1)
S = 50.0 * torch.randn(N, 3, 3, generator=gen)
colliders = [
    dict(type="plane", point=[0.5, 0.45, 0.5], normal=[0.2, 1, 0], surface="friction", friction=0.4),
    dict(type="plane", point=[0.4, 0.5, 0.5], normal=[1, 0.1, 0], surface="slip"),
    dict(type="plane", point=[0.5, 0.5, 0.62], normal=[0, 0.1, -1], surface="sticky"),
    dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.12, surface="friction", friction=0.3, velocity=[0, 0.1, 0]),
    dict(type="sphere", center=[0.6, 0.6, 0.4], radius=0.1, surface="slip"),
    dict(type="sphere", center=[0.4, 0.6, 0.6], radius=0.08, surface="sticky"),
    dict(type="box", center=[0.55, 0.4, 0.45], half=[0.1, 0.05, 0.1], euler_xyz_deg=[10, 20, 30], surface="friction", friction=0.5),
    dict(type="box", center=[0.45, 0.6, 0.55], half=[0.06, 0.06, 0.06], euler_xyz_deg=[0, 0, 20], surface="slip"),
]
cfg = dict(gravity=[0.0, -9.8, 0.0], bc="freeslip", num_grids=G, dt=1e-4, bound=3, eps=6e-7)
lib = L.lib()
for tag, cs in (("no colliders", []), ("8 colliders", colliders)):
    model = MPMModelBuilder().parse_cfg(dict(cfg, colliders=cs)).finalize(dev, requires_grad=True)
    model.grid_cache = 0      # recompute path: every k_grid_op launch does the whole update (none returns at once on a valid record)
    st = model.statics(N)
    st.vol.fill_((1.0 / G / 2) ** 3); st.rho.fill_(1000.0); st.clip_bound.fill_(0.5); st.enabled.fill_(1)
    sim = MPMDiffSim(model, reorder=False)

    def step():
        ins = [t.to(dev).requires_grad_(True) for t in (x, v, Cm, F, S)]
        outs = sim(st, *ins)
        torch.autograd.grad(sum(o.sum() for o in outs), ins)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    lib.nm_prof_reset(); lib.nm_prof_enable(1, None)
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    lib.nm_prof_enable(0, None)
    buf = C.create_string_buffer(1 << 16)
    lib.nm_prof_report(buf, len(buf))
    rows = {r.split()[0]: (int(r.split()[1]), float(r.split()[2])) for r in buf.value.decode().splitlines() if r.strip()}
    blocks, nodes = model.grid_stats()
    print(f"{tag}: N={N} G={G} active blocks {blocks}, nodes with mass {nodes}, {iters} substeps forward + backward")
    for k in ("k_grid_op", "k_grid_collide", "k_grid_op_bwd", "k_grid_collide_bwd"):
        if k in rows:
            print(f"  {k:20s} {rows[k][0]:5d} launches  {1e3 * rows[k][1] / rows[k][0]:8.2f} us each")
        else:
            print(f"  {k:20s}     0 launches")
