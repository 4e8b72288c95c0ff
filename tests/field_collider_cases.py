"""Cases of the field-collider tests, chosen WITHOUT a GPU: a mesh (tests/mesh_sdf_cases.py), a lattice, the fp64 CPU field on it
rounded to fp32 (the data both the definition and the kernels read), and the checks that the fp64 reference of a case sits away
from every branch fp32 may decide otherwise.

Lattices: "dyadic" - origin a multiple of 1/64 and spacing 1/32, so q = (p - origin) / spacing is exact in fp32 for the grid
nodes of G = 16, 32 (they sit exactly on lattice planes: t = 0 in both precisions) - and "odd": an origin and a spacing that are
nothing in particular (rounded to fp32 once: the definition and the kernels see the same numbers)."""
import functools

import numpy as np
import torch

import mesh_sdf_cases as cases
from gpu_util import mpm_case
from neuma_amd.extras import colliders as xc
from neuma_amd.extras import mesh_sdf as X
from neuma_amd.extras import mesh_sampling as ms
from neuma_amd.sim.colliders import FieldCollider
from oracle import mpm as om

SIZES = [(4096, 32), (3001, 16)]
VC = (0.0531, 0.0217, -0.0293)      # the collider velocity of tests/test_gpu_colliders.py
MU = 0.4
PHI_MARGIN = 1e-5                   # no node with mass has |phi| below it (simulation units; |phi| is of order 0.1)
T_MARGIN = 1e-5                     # ... or, on the odd lattice, a fraction t_a this close to a cell face
EXCLUDE_CAP = 0.01                  # of the nodes with mass, should a case not be clean (none of the cases here needs it)
# bounds of the collider-free substep (tests/test_gpu_mpm.py, tests/test_gpu_colliders.py)
BOUNDS = {"grid v (mass-weighted)": 7e-7, "x": 1e-7, "v": 7e-7, "C": 1e-6, "F": 7e-7}
ADJ_BOUND = 8e-6
# pose of each mesh: a small shift of tests/mesh_sdf_cases.py's, chosen on the CPU so that every case below is clean (assert_clean)
SHIFT = {"torus": (0.011, 0.009, -0.007), "box": (0.007, -0.004, 0.005)}


def mesh(name):
    v, t = cases.MESHES[name]()
    return v + np.asarray(SHIFT[name]), t


def lattice(kind, verts):
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    if kind == "dyadic":
        h = 1.0 / 32
        origin = np.floor((lo - 2 * h) * 64) / 64
    else:
        h = float(np.float32(0.0271))
        origin = (lo - 2.3 * h + np.array([0.0013, 0.0007, 0.0021])).astype(np.float32).astype(np.float64)
    dims = tuple(int(d) for d in np.ceil((hi + 2 * h - origin) / h).astype(int) + 1)
    return origin, h, dims


@functools.lru_cache(maxsize=None)
def field(name, kind):
    """(phi (nx, ny, nz) fp32 numpy, origin, spacing, dims): the CPU field of the mesh on the lattice, computed once"""
    v, t = mesh(name)
    origin, h, dims = lattice(kind, v)
    assert all(float(np.float32(o)) == o for o in origin) and float(np.float32(h)) == h
    dist = X.mesh_distance(v, t, origin.astype(np.float32), np.float32(h), dims)
    v32 = np.asarray(v, dtype=np.float32).astype(np.float64)
    inside = ms.points_in_mesh(X.lattice_nodes(origin, h, dims).reshape(-1, 3), v32, X.kept_triangles(len(v), t)).reshape(dims)
    phi = np.where(inside, -dist, dist).astype(np.float32)
    phi.setflags(write=False)
    return phi, tuple(float(o) for o in origin), h, dims


def collider(name, kind, surface, velocity=VC, phi=None):
    f, origin, h, dims = field(name, kind)
    return FieldCollider(surface=surface, friction=MU if surface == "friction" else 0.0, velocity=velocity,
                         phi=f if phi is None else phi, origin=origin, spacing=h, dims=dims)


@functools.lru_cache(maxsize=None)
def mpm_grid(N, G, bc, seed=0):
    """mpm_case rounded to fp32 (what the GPU sees) and the oracle's grid behind the box boundary condition, as
    tests/test_gpu_colliders.py _case: computed once per (size, bc, seed), shared, never modified"""
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=N, G=G, bc=bc, seed=seed)
    ins = tuple(t.float().double() for t in (x, v, C_, F, S))
    gmv, gm = om.p2g(const, vol, rho, en, ins[0], ins[1], ins[2], ins[4])
    gv = om.grid_op(const, gmv, gm)
    return const, (vol, rho, clip, en), ins, (gmv, gm, gv)


def unsafe_nodes(cs, gv, gm, G, kind, with_mass=True):
    """fp64 alone: (G^3,) bool, the nodes WITH MASS (with_mass=False: all nodes) that sit at a branch - |phi| < PHI_MARGIN on a lattice; on the odd lattice a
    fraction within T_MARGIN of a cell face; inside a collider at a jump of the response's Jacobian (_check_thresholds of
    tests/test_gpu_colliders.py: |vn| < 1e-4 |w|, |vt| < 1e-4 |w|, friction within 1e-4 of the edge of the Coulomb cone)."""
    p = xc.node_positions(G)
    u = gv.reshape(-1, 3)
    bad = torch.zeros(G ** 3, dtype=torch.bool)
    kinds = [kind] * len(cs) if isinstance(kind, str) else list(kind)
    for c, kind in zip(cs, kinds):
        inside, phi, n = xc.field_phi_normal(c, p)
        q = (p - torch.tensor(c.origin, dtype=p.dtype)) / c.spacing
        on = ((q >= 0) & (q <= torch.tensor(c.dims) - 1)).all(-1)
        bad |= on & (phi.abs() < PHI_MARGIN)
        if kind != "dyadic":
            t = q - q.floor()
            bad |= on & ((t < T_MARGIN) | (t > 1 - T_MARGIN)).any(-1)
            edge = ((q < T_MARGIN) & (q > -T_MARGIN)) | (((q - (torch.tensor(c.dims) - 1)).abs()) < T_MARGIN)      # on / off the lattice
            bad |= edge.any(-1)
        w = u - torch.tensor(c.velocity, dtype=u.dtype)
        vn = (w * n).sum(-1)
        vt = w - vn[:, None] * n
        s, wl = vt.norm(dim=-1), w.norm(dim=-1)
        jump = (vn.abs() < 1e-4 * wl) | (s < 1e-4 * wl)
        if c.surface == "friction":
            jump |= (vn < 0) & ((1.0 + c.friction * vn / s.clamp_min(1e-300)).abs() < 1e-4)
        bad |= inside & jump
        u = xc.apply_field_collider(c, p, u)
    return bad & (gm.reshape(-1) > 0) if with_mass else bad


def assert_clean(cs, gv, gm, G, kind):
    """the condition, not a measurement: no node with mass at a branch; and the collider holds nodes with mass"""
    bad = unsafe_nodes(cs, gv, gm, G, kind)
    massy = int((gm.reshape(-1) > 0).sum())
    assert int(bad.sum()) <= EXCLUDE_CAP * massy, f"{int(bad.sum())} of {massy} nodes with mass sit at a branch"
    assert int(bad.sum()) == 0, "this case was chosen to be clean"
    inside = xc.field_phi_normal(cs[0], xc.node_positions(G))[0]
    assert int((inside & (gm.reshape(-1) > 0)).sum()) >= 8, "the collider holds (almost) no node with mass"
