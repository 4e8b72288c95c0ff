"""The contact report as a torch function over the dense grid of one substep: the DEFINITION the native reduction
(csrc/nm_contact.h, k_contact_rows / k_contact_sum, nm_mpm_contact) is held to.  Prose: include/neuma_hip.h "Contact report".

    rows, scale = contact_rows(mv, m, dt=..., gravity=..., eps=..., bound=..., bc=..., num_grids=..., colliders=[...])

mv (G, G, G, 3) / (G^3, 3) node momentum and m (G, G, G) / (G^3,) node mass of the substep; `colliders` the list exactly as it is
applied (analytic first, then FieldCollider objects).  At every node with m > 0, at p = (i, j, k) / G:

    u^(0) = mv / (m + eps) + g dt            u_free
    u^(1) = BC(u^(0))                        the box boundary condition (`box_bc`)
    u^(c+1) = apply_collider(c, p, u^(c))    extras/colliders.py, in list order

Row r (0: the box walls, r >= 1: collider r) is the impulse the body hands to obstacle r in this substep, nine numbers:

    J[3]   sum m (u^(r) - u^(r+1))
    L[3]   sum m p x (u^(r) - u^(r+1))                 about the simulation origin
    N      sum_inside m (u^(r+1) - u^(r)) . n          n the collider's outward normal; 0 in the walls row
    mass   sum_inside m                                walls: the boundary layers (an index < bound or >= G - bound on any axis)
    nodes  the number of those nodes

A collider that is a rigid body (extras/rigid.py) goes in at its current pose (rigid.posed) with its angular velocity in
`omegas`, one entry per collider (None for the others): its own velocity at a node is then v + w x (p - c).

`scale` (R,) is S_r = sum_inside m (|u^(r)| + |u^(r+1)|), what a parity test divides an error of row r by.  Everything is fp64.
Units are simulation units (the unit cube, rho * vol masses).  force() / torque() derive F = J / dt and (L - r0 x J) / dt.
Not on the product path: nothing here is called by a simulation, and nothing here imports the test oracle.
"""
from typing import Sequence, Tuple

import torch
from torch import Tensor

from ..sim.colliders import FieldCollider
from . import colliders as xc

COLS = 9
J, L, N, MASS, NODES = slice(0, 3), slice(3, 6), 6, 7, 8


def free_velocity(mv: Tensor, m: Tensor, dt: float, gravity, eps: float) -> Tensor:
    """u^(0) (M, 3) of mv (M, 3), m (M,): mv / (m + eps) + g dt where m > 0, g dt elsewhere (as grid_velocity)."""
    g = torch.as_tensor(gravity, dtype=mv.dtype).reshape(3) * dt
    has = m > 0
    safe = torch.where(has, m, torch.ones_like(m))
    return torch.where(has[:, None], mv / (safe + eps)[:, None] + g, g.expand_as(mv))


def boundary_layer(num_grids: int, bound: int) -> Tuple[Tensor, Tensor]:
    """((G^3, 3) bool low layers, (G^3, 3) bool high layers): per axis, index < bound / index >= G - bound."""
    idx = (xc.node_positions(num_grids) * num_grids).round().long()
    return idx < bound, idx >= num_grids - bound


def box_bc(u: Tensor, num_grids: int, bound: int, bc: str) -> Tensor:
    """The box boundary condition on u (G^3, 3): a component that points out of the box in a boundary layer is a hit; freeslip
    zeroes that component, noslip the whole vector."""
    lo, hi = boundary_layer(num_grids, bound)
    hit = (lo & (u < 0)) | (hi & (u > 0))
    if bc == "freeslip":
        return torch.where(hit, torch.zeros_like(u), u)
    if bc == "noslip":
        return torch.where(hit.any(-1, keepdim=True), torch.zeros_like(u), u)
    raise ValueError("invalid boundary condition: {}".format(bc))


def collider_inside_normal(c, p: Tensor) -> Tuple[Tensor, Tensor]:
    """((M,) bool inside, (M, 3) outward normal) of an analytic or field collider at the points p"""
    if isinstance(c, FieldCollider):
        inside, _, n = xc.field_phi_normal(c, p)
        return inside, n
    sdf, n = xc.sdf_normal(c, p)
    return sdf < 0, n


def contact_chain(mv: Tensor, m: Tensor, *, dt: float, gravity, eps: float, bound: int, bc: str, num_grids: int,
                  colliders: Sequence = (), omegas: Sequence = ()):
    """[u^(0), u^(1), ..., u^(R)] (each (G^3, 3) fp64; R = 1 + len(colliders)): the velocities along the chain at EVERY node."""
    G = int(num_grids)
    mv = torch.as_tensor(mv).detach().cpu().double().reshape(G ** 3, 3)
    m = torch.as_tensor(m).detach().cpu().double().reshape(G ** 3)
    p = xc.node_positions(G)
    chain = [free_velocity(mv, m, float(dt), gravity, float(eps))]
    chain.append(box_bc(chain[0], G, int(bound), bc))
    for i, c in enumerate(colliders):
        chain.append(xc.apply_collider(c, p, chain[-1]) if not omegas or omegas[i] is None
                     else xc.apply_collider(c, p, chain[-1], omegas[i]))
    return chain


def contact_rows(mv: Tensor, m: Tensor, *, dt: float, gravity, eps: float, bound: int, bc: str, num_grids: int,
                 colliders: Sequence = (), omegas: Sequence = ()) -> Tuple[Tensor, Tensor]:
    """(rows (R, 9) fp64, scale (R,) fp64), R = 1 + len(colliders): see the module docstring."""
    G = int(num_grids)
    m = torch.as_tensor(m).detach().cpu().double().reshape(G ** 3)
    chain = contact_chain(mv, m, dt=dt, gravity=gravity, eps=eps, bound=bound, bc=bc, num_grids=G, colliders=colliders,
                          omegas=omegas)
    p = xc.node_positions(G)
    has = m > 0
    mm = torch.where(has, m, torch.zeros_like(m))
    rows = torch.zeros(len(chain) - 1, COLS, dtype=torch.float64)
    scale = torch.zeros(len(chain) - 1, dtype=torch.float64)
    for r in range(len(chain) - 1):
        a, b = chain[r], chain[r + 1]
        if r == 0:
            lo, hi = boundary_layer(G, int(bound))
            inside, n = (lo | hi).any(-1), torch.zeros_like(p)
        else:
            inside, n = collider_inside_normal(colliders[r - 1], p)
        inside = inside & has
        d = mm[:, None] * (a - b)
        rows[r, J] = d.sum(0)
        rows[r, L] = torch.linalg.cross(p, d).sum(0)
        rows[r, N] = -(d * n)[inside].sum()
        rows[r, MASS] = mm[inside].sum()
        rows[r, NODES] = float(inside.sum())
        scale[r] = (mm * (a.norm(dim=-1) + b.norm(dim=-1)))[inside].sum()
    return rows, scale


def force(rows: Tensor, dt: float) -> Tensor:
    """(R, 3): F = J / dt, the mean force on each obstacle over the time dt the impulses were gathered in"""
    return rows[..., J] / dt


def torque(rows: Tensor, dt: float, about) -> Tensor:
    """(R, 3): (L - r0 x J) / dt, r0 = `about` (3,) or one point per row (R, 3)"""
    r0 = torch.as_tensor(about, dtype=rows.dtype, device=rows.device).expand_as(rows[..., J])
    return (rows[..., L] - torch.linalg.cross(r0, rows[..., J])) / dt
