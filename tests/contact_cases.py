"""Cases of the contact-report tests (tests/test_contact_cpu.py, tests/test_gpu_contact.py), chosen WITHOUT a GPU: the collider
placements of tests/test_gpu_colliders.py and tests/field_collider_cases.py on the grids of gpu_util.mpm_case, and the fp64 checks
that a case sits away from every branch fp32 may decide otherwise (the inside test, the box's face choice, the field's cell).
The responses themselves are continuous in u, so the sums compared here need no velocity thresholds."""
import functools

import torch

import field_collider_cases as fcc
from gpu_util import mpm_case
from neuma_amd.extras import colliders as xc
from neuma_amd.extras import contact as xk
from neuma_amd.sim.colliders import Sphere, parse_colliders
from test_gpu_colliders import MU, SIZES, VC, _case, _check_geometry, collider_cfg

BOUND = 7e-7      # mass-weighted node velocities of these very cases: tests/test_gpu_colliders.py, field_collider_cases.BOUNDS
assert BOUND == fcc.BOUNDS["grid v (mass-weighted)"]
BCS = ["noslip", "freeslip"]
SHAPES = ["plane", "sphere", "box"]
SURFACES = ["sticky", "slip", "friction"]


def const_kwargs(const):
    return dict(dt=const.dt, gravity=const.gravity, eps=const.eps, bound=const.bound, bc=const.bc, num_grids=const.num_grids)


def twin(const, mv, m, colliders):
    """(rows (R, 9), scale (R,)) of the fp64 definition on the grid {mv, m} (any dtype / device: taken to fp64 on the CPU)"""
    return xk.contact_rows(mv, m, colliders=list(colliders), **const_kwargs(const))


def single(shape, surface, G):
    cs = parse_colliders([collider_cfg(shape, surface, G)])
    _check_geometry(cs, G)
    return cs


def pair(G):
    """[plane / friction, sphere / slip]: the two overlap, so the order of the chain matters (nodes_in_both)"""
    cs = parse_colliders([collider_cfg("plane", "friction", G), collider_cfg("sphere", "slip", G)])
    _check_geometry(cs, G)
    return cs


def nodes_in_both(cs, gm, G):
    p = xc.node_positions(G)
    both = torch.ones(G ** 3, dtype=torch.bool)
    for c in cs:
        both &= xk.collider_inside_normal(c, p)[0]
    return int((both & (gm.reshape(-1) > 0)).sum())


def analytic_and_field(N, G, bc):
    """[sphere / slip, torus field / friction] of tests/test_gpu_field_colliders.py's list-order case, with its margins asserted on
    this grid: the sphere's by _check_geometry, the field's by assert_clean on the velocities behind the sphere"""
    _, _, _, (_, gm, gv) = _case(N, G, bc)
    sph = Sphere(center=(0.5, 0.5, 0.5), radius=0.12, surface="slip", velocity=fcc.VC)
    cs = [sph, fcc.collider("torus", "dyadic", "friction")]
    _check_geometry(cs[:1], G)
    fcc.assert_clean(cs[1:], xc.apply_colliders([sph], gv, G), gm, G, ["dyadic"])
    return cs


@functools.lru_cache(maxsize=None)
def padding_case():
    """mpm_case(N=1000, G=10): the 3 x 3 x 3 blocks of 4 x 4 x 4 nodes cover 12 per axis, so every edge block has padding lanes.
    Rounded to fp32 (what the GPU sees); computed once, never modified."""
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=1000, G=10)
    return const, (vol, rho, clip, en), tuple(t.float().double() for t in (x, v, C_, F, S))


def padding_sphere(surface):
    """centre (0.5, 0.5, 0.5), radius 0.15 at G = 10: 19 nodes inside, the nearest node 0.086 dx from the surface (asserted: > 0.05)"""
    cs = parse_colliders([dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.15, surface=surface,
                               friction=MU if surface == "friction" else 0.0, velocity=list(VC))])
    _check_geometry(cs, 10)
    return cs


def momentum(vol, rho, en, v):
    """sum over the enabled particles of m_p v_p, fp64 (3,)"""
    mp = (vol.double() * rho.double())[en != 0]
    return (mp[:, None] * v.detach().cpu().double()[en != 0]).sum(0)
