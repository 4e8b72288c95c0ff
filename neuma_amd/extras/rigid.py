"""Rigid bodies in fp64 numpy: the DEFINITION the native step (csrc/nm_rigid.h, k_rigid_step, nm_mpm_rigid_step) and the body
variants of the collide / contact kernels are held to.  Prose: include/neuma_hip.h "Rigid bodies".

A body is a Sphere or Box (sim/colliders.py) with a RigidBody record: mass M, body-frame principal inertia I_b, flags.  Its state
is centre c, unit quaternion q (wxyz), linear momentum P and angular momentum Lc about the centre, in simulation axes;
v = P / M and w = R(q) diag(1 / I_b) R(q)^T Lc (a kinematic body keeps the angular velocity it was given).  At a grid node at p the
body's own velocity is v + w x (p - c) (`body_velocity`; extras/colliders.py apply_collider takes it through `omega`).

    state = initial_state(collider)                         from center, rot, velocity, body.angular_velocity
    state = rigid_step(state, row, collider.body, dt, g)    one symplectic-Euler step; row: the body's contact row (J, L about
                                                            the origin; extras/contact.py), or None for no contact at all
    posed(collider, state)                                  the Sphere / Box at the state's pose, velocity v, for apply_collider

    P  += J + M g dt;   Lc += L - c x J (the old c);   c += (P / M) dt;   q <- normalize(exp(w dt / 2) (x) q)

with the new w through R of the old q, and the exact exponential (cos(theta/2), sin(theta/2) w / |w|), theta = |w| dt
(sin(theta/2)/theta from its series below SERIES_BELOW).  Not on the product path: nothing here is called by a simulation, and
nothing here imports the test oracle.
"""
import math
from dataclasses import dataclass, replace
from typing import Optional, Sequence, Tuple

import numpy as np

from ..sim.colliders import Box, RigidBody, Sphere, principal_inertia

SERIES_BELOW = 1e-2      # theta below which sin(theta/2)/theta = 1/2 - theta^2/48 + theta^4/3840 (next term < 2^-53 of the first)
STATE_COLS = 19          # c[3], q[4], P[3], Lc[3], v[3], w[3]: a row of MPMModel.rigid_state()


@dataclass
class RigidState:
    c: np.ndarray       # (3,)
    q: np.ndarray       # (4,) wxyz, unit
    P: np.ndarray       # (3,)
    Lc: np.ndarray      # (3,)

    @classmethod
    def from_row(cls, row) -> "RigidState":
        """from one row of MPMModel.rigid_state() (its first 13 numbers)"""
        r = np.asarray(row, dtype=np.float64).reshape(-1)
        return cls(r[0:3].copy(), r[3:7].copy(), r[7:10].copy(), r[10:13].copy())


def inertia(shape, mass: float) -> np.ndarray:
    """Body-frame principal inertia of a solid Sphere (2/5 M r^2) or Box (M/3 (hy^2 + hz^2, hx^2 + hz^2, hx^2 + hy^2))."""
    return np.asarray(principal_inertia(shape, float(mass)), dtype=np.float64)


def quat_rot(q) -> np.ndarray:
    """R(q) (3, 3) of a unit quaternion (w, x, y, z)"""
    w, x, y, z = (float(a) for a in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def rot_quat(R) -> np.ndarray:
    """the unit quaternion (w, x, y, z) of a rotation matrix, by the largest of the four squared components"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q, dtype=np.float64)
    return q / math.sqrt(float(q @ q))


def body_velocity(c, v, w, p) -> np.ndarray:
    """v + w x (p - c) at the points p (M, 3) (or one point (3,))"""
    p = np.asarray(p, dtype=np.float64)
    return np.asarray(v, dtype=np.float64) + np.cross(np.asarray(w, dtype=np.float64), p - np.asarray(c, dtype=np.float64))


def velocities(state: RigidState, body: RigidBody) -> Tuple[np.ndarray, np.ndarray]:
    """(v, w) of a body as it stands"""
    v = state.P / body.mass
    if body.kinematic:
        return v, np.asarray(body.angular_velocity, dtype=np.float64)
    R = quat_rot(state.q)
    return v, R @ ((R.T @ state.Lc) / np.asarray(body.inertia, dtype=np.float64))


def initial_state(collider, fp32: bool = True) -> RigidState:
    """The state nm_mpm_set_rigid_bodies builds from a body's Sphere / Box: `fp32` takes center, rot and velocity through the
    fp32 values of nm_collider, as the library sees them."""
    body = collider.body
    cast = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if fp32 else (lambda a: np.asarray(a, dtype=np.float64))
    R = cast(collider.rot).reshape(3, 3) if isinstance(collider, Box) else np.eye(3)
    q = rot_quat(R)
    R = quat_rot(q)
    w = np.asarray(body.angular_velocity, dtype=np.float64)
    Lc = R @ ((R.T @ w) * np.asarray(body.inertia, dtype=np.float64))
    return RigidState(cast(collider.center), q, body.mass * cast(collider.velocity), Lc)


def rotate(q, w, dt: float) -> np.ndarray:
    """normalize(exp(w dt / 2) (x) q)"""
    w = np.asarray(w, dtype=np.float64)
    th = math.sqrt(float(w @ w)) * dt
    t2 = th * th
    k = (0.5 - t2 / 48.0 + t2 * t2 / 3840.0 if th < SERIES_BELOW else math.sin(0.5 * th) / th) * dt
    e = np.array([math.cos(0.5 * th), k * w[0], k * w[1], k * w[2]])
    r = np.array([e[0] * q[0] - e[1] * q[1] - e[2] * q[2] - e[3] * q[3], e[0] * q[1] + e[1] * q[0] + e[2] * q[3] - e[3] * q[2],
                  e[0] * q[2] - e[1] * q[3] + e[2] * q[0] + e[3] * q[1], e[0] * q[3] + e[1] * q[2] - e[2] * q[1] + e[3] * q[0]])
    return r / math.sqrt(float(r @ r))


def rigid_step(state: RigidState, rows, consts: RigidBody, dt: float, gravity) -> RigidState:
    """One step of one body.  rows: its contact row (at least J[3], L[3] about the origin; extras/contact.py), or None - no contact,
    and then Lc is not touched at all.  gravity: the model's g (3,); it acts unless consts.gravity is off."""
    c, q, P, Lc = state.c.copy(), state.q.copy(), state.P.copy(), state.Lc.copy()
    if not consts.kinematic:
        if rows is not None:
            r = np.asarray(rows, dtype=np.float64).reshape(-1)
            J, L = r[0:3], r[3:6]
            P = P + J
            Lc = Lc + (L - np.cross(c, J))
        if consts.gravity:
            P = P + consts.mass * np.asarray(gravity, dtype=np.float64) * dt
    nxt = RigidState(c, q, P, Lc)
    v, w = velocities(nxt, consts)
    nxt.c = c + v * dt
    nxt.q = rotate(q, w, dt)
    return nxt


def kinetic_energy(state: RigidState, body: RigidBody) -> float:
    v, w = velocities(state, body)
    return 0.5 * body.mass * float(v @ v) + 0.5 * float(w @ state.Lc)


def posed(collider, state: RigidState):
    """(the Sphere / Box at the state's pose with velocity v, w): what apply_collider(c, p, u, omega=w) takes"""
    v, w = velocities(state, collider.body)
    kw = dict(center=tuple(float(a) for a in state.c), velocity=tuple(float(a) for a in v))
    if isinstance(collider, Box):
        kw["rot"] = tuple(float(a) for a in quat_rot(state.q).reshape(-1))
    elif not isinstance(collider, Sphere):
        raise TypeError(f"not a rigid body's shape: {collider!r}")
    return replace(collider, **kw), w
