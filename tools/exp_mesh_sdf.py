"""Cost of the mesh distance kernel and of the field-collider kernels ("Mesh colliders").

Part 1 - nm_mesh_distance (csrc/nm_sdf.hip) on a 128^3 lattice for a sphere of 5 120 triangles and a torus of 72 200, with the
triangles in three orders: as generated, in Morton order of their centroids, and in the fixed pseudo-random order
neuma_amd.mesh_sdf uploads them in (extras.mesh_sdf.cull_order).
Device events around `reps` back-to-back calls after `warm` calls, `rounds` times; median and spread are printed.  Next to it
the yardstick: the same formula as chunked torch tensor operations on the same device (extras/mesh_sdf.py pair_dist2, restated
in torch below), on the first `BF_NODES` lattice nodes and scaled to the lattice by the node count; the largest difference
between the two results on those nodes is printed too.

Part 2 - k_grid_collide_field / k_grid_collide_field_bwd on the 100 000-particle / 128^3 case of tools/exp_colliders.py with four
mesh colliders that all cut the body, next to k_grid_op / k_grid_op_bwd of the same run (nm_prof_enable(1): every launch timed).

    python tools/exp_mesh_sdf.py [reps] [rounds]"""
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from neuma_amd import _lib as L, mesh_sdf                                           # noqa: E402
from neuma_amd.extras import mesh_sdf as X                                          # noqa: E402
from neuma_amd.sim import MPMDiffSim, MPMModelBuilder                               # noqa: E402
import mesh_sdf_cases as cases                                                      # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warm = 2
DIMS = (128, 128, 128)
BF_NODES = 1 << 16
assert torch.cuda.is_available(), "needs a GPU (no CPU timing)"
dev = torch.device("cuda", 0)
lib = L.lib()


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms per call


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def torch_dist2(p, a, ab, ac):
    """extras/mesh_sdf.py pair_dist2 for non-degenerate triangles, as torch operations: p (M, 3) -> (M,) min over the triangles"""
    aa, bb, cc = dot(ab, ab), dot(ab, ac), dot(ac, ac)
    ap = p[:, None, :] - a[None]
    d1, d2 = dot(ab[None], ap), dot(ac[None], ap)
    d3, d4, d5, d6 = d1 - aa, d2 - bb, d1 - bb, d2 - cc
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    e43, e56 = d4 - d3, d5 - d6
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    nv, nw, den = vb, vc, (va + vb) + vc
    for m, rv, rw, rd in (((va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                          ((d6 >= 0) & (d5 <= d6), zero, one, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                          ((d3 >= 0) & (d4 <= d3), one, zero, one), ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
        nv, nw, den = torch.where(m, rv, nv), torch.where(m, rw, nw), torch.where(m, rd, den)
    r = 1.0 / den
    e = (ab[None] * (nv * r)[..., None] + ac[None] * (nw * r)[..., None]) - ap
    return dot(e, e).min(dim=1).values


def morton_order(verts, tris) -> np.ndarray:
    """permutation of the triangles by the 30-bit Morton code of their centroids (10 bits per axis over the mesh's box)"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return np.zeros(0, dtype=np.int64)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    cen = v[np.clip(t, 0, max(len(v) - 1, 0))].mean(axis=1)
    lo, hi = cen[ok].min(0) if ok.any() else np.zeros(3), cen[ok].max(0) if ok.any() else np.ones(3)
    q = np.clip((cen - lo) / np.maximum(hi - lo, 1e-300) * 1023.0, 0, 1023).astype(np.uint64)
    code = np.zeros(len(t), dtype=np.uint64)
    for bit in range(10):
        for k in range(3):
            code |= ((q[:, k] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + k)
    return np.argsort(code, kind="stable")


def big_torus(nu=190, nv=190):
    return cases.torus(nu, nv)


def sphere(level=4):
    v, t = cases.icosahedron()
    for _ in range(level):
        v, t = cases.subdivide(v, t, 0.3, (0.5, 0.45, 0.55))
    return v, t


print(f"nm_mesh_distance, lattice {DIMS[0]}^3; {reps} calls per round, {rounds} rounds, {warm} warm-up calls")
for name, (v, t) in (("sphere", sphere()), ("torus", big_torus())):
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    lo, hi = v.min(0) - 0.05, v.max(0) + 0.05
    h = np.float32(float((hi - lo).max()) / (DIMS[0] - 1))
    origin = lo.astype(np.float32)
    vd = torch.from_numpy(v32).to(dev)
    results = {}
    for order, perm in (("as generated", np.arange(len(t))), ("Morton", morton_order(v, t)),
                        ("cull_order", X.cull_order(len(t)))):
        td = torch.from_numpy(np.ascontiguousarray(t[perm], dtype=np.int32)).to(dev)
        out = torch.empty(DIMS, dtype=torch.float32, device=dev)
        fn = lambda: mesh_sdf.distance_native(vd, td, origin, h, DIMS, out=out)      # noqa: E731
        timed(fn, warm)
        ms = [timed(fn, reps) for _ in range(rounds)]
        results[order] = out.clone()
        pairs = DIMS[0] ** 3 * len(t)
        print(f"  {name} {len(t):6d} triangles, {order:12s}: {statistics.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"
              f"  = {pairs / statistics.median(ms) / 1e6:9.1f} G node-triangle pairs/s of the uncut product")
    assert all(torch.equal(results["cull_order"], r) for r in results.values()), "the field depends on the triangle order"
    # the yardstick on the first BF_NODES nodes
    a = torch.from_numpy(v32[t[:, 0]]).to(dev)
    ab, ac = torch.from_numpy(v32[t[:, 1]]).to(dev) - a, torch.from_numpy(v32[t[:, 2]]).to(dev) - a
    nodes = torch.from_numpy(X.lattice_nodes(origin, h, DIMS, np.float32).reshape(-1, 3)[:BF_NODES]).to(dev)
    chunk = max(64, min(4096, (1 << 26) // len(t)))

    def brute():
        return torch.cat([torch_dist2(nodes[i:i + chunk], a, ab, ac) for i in range(0, BF_NODES, chunk)]).sqrt()

    timed(brute, 1)
    bf = [timed(brute, 1) for _ in range(3)]
    scale = DIMS[0] ** 3 / BF_NODES
    diff = float((brute() - results["cull_order"].reshape(-1)[:BF_NODES]).abs().max())
    print(f"  {name} torch brute force ({chunk} nodes per chunk): {statistics.median(bf):9.3f} ms for {BF_NODES} nodes -> "
          f"{statistics.median(bf) * scale:10.1f} ms scaled to the lattice; max |kernel - torch| on those nodes {diff:.2e}")

# ---- part 2: the collide kernels
N, G = 100_000, 128
iters = 30
gen = torch.Generator().manual_seed(0)
x = 0.3 + 0.4 * torch.rand(N, 3, generator=gen)
cell = torch.floor(x * G).long()
x = x[torch.argsort((cell[:, 0] * G + cell[:, 1]) * G + cell[:, 2])].contiguous()
v = torch.randn(N, 3, generator=gen)
Cm = torch.zeros(N, 3, 3)
F = torch.eye(3).repeat(N, 1, 1)
S = 50.0 * torch.randn(N, 3, 3, generator=gen)
meshes = [("torus", "friction"), ("box", "slip"), ("sphere320", "sticky"), ("icosahedron", "friction")]
colliders = [dict(type="mesh", verts=cases.MESHES[m]()[0], tris=cases.MESHES[m]()[1], resolution=64, surface=s,
                  friction=0.4 if s == "friction" else 0.0, velocity=[0, 0.1 * i, 0]) for i, (m, s) in enumerate(meshes)]
cfg = dict(gravity=[0.0, -9.8, 0.0], bc="freeslip", num_grids=G, dt=1e-4, bound=3, eps=6e-7)
for tag, cs in (("no colliders", []), ("4 mesh colliders", colliders)):
    model = MPMModelBuilder().parse_cfg(dict(cfg, colliders=cs)).finalize(dev, requires_grad=True)
    model.grid_cache = 0      # recompute path: every k_grid_op launch does the whole update
    st = model.statics(N)
    st.vol.fill_((1.0 / G / 2) ** 3); st.rho.fill_(1000.0); st.clip_bound.fill_(0.5); st.enabled.fill_(1)
    sim = MPMDiffSim(model, reorder=False)

    def step():
        ins = [t_.to(dev).requires_grad_(True) for t_ in (x, v, Cm, F, S)]
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
    blocks, nodes_m = model.grid_stats()
    print(f"{tag}: N={N} G={G} active blocks {blocks}, nodes with mass {nodes_m}, {iters} substeps forward + backward"
          + "".join(f"; lattice {'x'.join(map(str, c.dims))}" for c in model.field_colliders))
    for k in ("k_grid_op", "k_grid_collide_field", "k_grid_op_bwd", "k_grid_collide_field_bwd"):
        if k in rows:
            print(f"  {k:26s} {rows[k][0]:5d} launches  {1e3 * rows[k][1] / rows[k][0]:8.2f} us each")
        else:
            print(f"  {k:26s}     0 launches")
