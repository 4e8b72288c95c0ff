"""Cases of the rigid-body tests (tests/test_rigid_cpu.py, tests/test_gpu_rigid.py), chosen WITHOUT a GPU: the sphere and box of
tests/test_gpu_colliders.py made rigid bodies on the grids of gpu_util.mpm_case, each with an angular velocity scaled on the CPU
so that the turning part of the body's velocity field, |w x (p - c)|, stays within |VC| at every node inside it - the response
then moves in the range the project's bound for these very cases (contact_cases.BOUND, at w = 0) was measured in.  The geometry
margins of those cases are asserted again at the pose the library holds (the box's rotation goes through its quaternion)."""
import math

import numpy as np
import torch

from contact_cases import BOUND, const_kwargs      # noqa: F401  (BOUND: re-exported to the tests)
from neuma_amd.extras import colliders as xc
from neuma_amd.extras import contact as xk
from neuma_amd.extras import rigid as xr
from neuma_amd.sim.colliders import parse_colliders
from test_gpu_colliders import MU, VC, _check_geometry, collider_cfg

SHAPES = ["sphere", "box"]
SURFACES = ["sticky", "slip", "friction"]
BCS = ["noslip", "freeslip"]
SIZES = [(3001, 16), (4096, 32)]
W_DIR = (0.36, -0.48, 0.8)      # a unit vector along no axis of the grid or of the box
MASS = 20.0                     # the 0.12 sphere holds about 1.7 (G = 32) / 10 (G = 16) of these clouds' mass: contact mass / M < 1
REL = 1e-12                     # fp64 results: the figure tests/test_gpu_contact.py holds the rows' mass column to


def inside(c, G):
    return xc.sdf_normal(c, xc.node_positions(G))[0] < 0


def omega_for(c, G, fill=0.9):
    """W_DIR scaled so that max over the nodes inside c of |w x (p - c)| is `fill` |VC|"""
    p = xc.node_positions(G)[inside(c, G)].numpy()
    arm = np.linalg.norm(np.cross(np.asarray(W_DIR), p - np.asarray(c.center)), axis=-1).max()
    return tuple(float(a) for a in np.asarray(W_DIR) * fill * math.sqrt(sum(v * v for v in VC)) / arm)


def body_cfg(shape, surface, G, kind="dynamic", velocity=VC, omega=None, **extra):
    """collider_cfg(shape, surface, G) as a rigid body entry of `sim.colliders`"""
    node = collider_cfg(shape, surface, G, velocity=velocity)
    plain = parse_colliders([node])[0]
    node = dict(node, **{kind: True}, angular_velocity=list(omega_for(plain, G) if omega is None else omega), **extra)
    if kind == "dynamic" and "mass" not in extra and "density" not in extra:
        node["mass"] = MASS
    return node


def bodies(nodes, G):
    """parse_colliders(nodes) with the geometry margins asserted at the pose the library starts the bodies from"""
    cs = parse_colliders(nodes)
    _check_geometry([xr.posed(c, xr.initial_state(c))[0] if c.body is not None else c for c in cs], G)
    for c in cs:
        if c.body is not None and any(c.body.angular_velocity):
            p = xc.node_positions(G)[inside(c, G)].numpy()
            turn = np.linalg.norm(np.cross(np.asarray(c.body.angular_velocity), p - np.asarray(c.center)), axis=-1).max()
            assert turn <= math.sqrt(sum(v * v for v in VC)) * (1 + 1e-12), "the body turns faster than |VC| at an inside node"
    return cs


def chain_pair(G):
    """[box / friction, sphere / sticky without gravity], both dynamic and turning, side by side: no node lies inside both (body -
    body contact is out of scope), and each holds nodes.  Margins are asserted for the box alone: the chained test feeds the twin
    the device's rows and never evaluates the sphere's geometry."""
    sph = dict(type="sphere", center=[0.640625, 0.640625, 0.34375], radius=0.0625, surface="sticky", dynamic=True, mass=MASS,
               velocity=list(VC), angular_velocity=[1.0, -0.5, 0.25], gravity=False)
    cs = bodies([body_cfg("box", "friction", G)], G) + parse_colliders([sph])
    a, b = inside(cs[0], G), inside(cs[1], G)
    assert int(b.sum()) >= 4 and not bool((a & b).any())
    return cs


def posed_list(cs, state_rows):
    """(colliders at the poses of `state_rows` (rows of MPMModel.rigid_state(), one per body in list order), omegas) for the twin"""
    out, omegas, rows = [], [], list(np.asarray(state_rows, dtype=np.float64))
    for c in cs:
        if c.body is None:
            out.append(c)
            omegas.append(None)
        else:
            pc, w = xr.posed(c, xr.RigidState.from_row(rows.pop(0)))
            out.append(pc)
            omegas.append(w)
    return out, omegas


def twin_rows(const, mv, m, cs, state_rows):
    pcs, omegas = posed_list(cs, state_rows)
    return xk.contact_rows(mv, m, colliders=pcs, omegas=omegas, **const_kwargs(const))


def twin_velocity(const, mv, m, cs, state_rows):
    """(G^3, 3) fp64 node velocities behind the whole chain on the grid {mv, m}"""
    pcs, omegas = posed_list(cs, state_rows)
    return xk.contact_chain(mv, m, colliders=pcs, omegas=omegas, **const_kwargs(const))[-1]


def device_dt_gravity(const):
    """dt and g as the handle holds them: fp32, widened"""
    return float(np.float32(const.dt)), np.asarray(const.gravity, dtype=np.float32).astype(np.float64)


def rel(a, b):
    """max |a - b| over max |b| (fp64 vectors)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def free_fall_centre(c0, v0, g, dt, n):
    """the symplectic-Euler centre after n free steps: c0 + n v0 dt + g dt^2 n (n + 1) / 2"""
    return np.asarray(c0) + n * dt * np.asarray(v0) + np.asarray(g) * dt * dt * (n * (n + 1) / 2)


def tensor(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)
