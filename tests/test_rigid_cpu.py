"""CPU: rigid bodies without a GPU - the `sim.colliders` keys and their refusals, the inertia formulas, the fp64 twin
(neuma_amd/extras/rigid.py) as a free body against its closed forms, and the default paths of the twins that gained an argument
(apply_collider(..., omega=None), contact_rows without bodies), which must return the bits they returned before."""
import math

import numpy as np
import pytest
import torch

import contact_cases as cc
import rigid_cases as rc
from neuma_amd.extras import colliders as xc
from neuma_amd.extras import contact as xk
from neuma_amd.extras import rigid as xr
from neuma_amd.sim import colliders as sc
from neuma_amd.sim.colliders import Box, RigidBody, Sphere, parse_colliders
from test_gpu_colliders import _case, collider_cfg

SPHERE = dict(type="sphere", center=[0.5, 0.6, 0.5], radius=0.1)
BOX = dict(type="box", center=[0.5, 0.6, 0.5], half=[0.1, 0.05, 0.2], euler_xyz_deg=[10, 20, 30])


@pytest.mark.parametrize("entry,field,text", [
    (dict(type="plane", dynamic=True, mass=1.0), "dynamic", "only a sphere or a box"),
    (dict(type="plane", kinematic=True), "kinematic", "only a sphere or a box"),
    (dict(type="mesh", path="x.obj", dynamic=True, mass=1.0), "dynamic", "only a sphere or a box"),
    (dict(SPHERE, dynamic=True), "mass", "needs mass or density"),
    (dict(SPHERE, dynamic=True, mass=0.0), "mass", "must be positive"),
    (dict(SPHERE, dynamic=True, mass=-2.0), "mass", "must be positive"),
    (dict(SPHERE, dynamic=True, mass=float("nan")), "mass", "must be positive"),
    (dict(SPHERE, dynamic=True, density=0.0), "density", "must be positive"),
    (dict(SPHERE, dynamic=True, mass=1.0, density=1.0), "density", "either mass or density"),
    (dict(SPHERE, dynamic=True, kinematic=True, mass=1.0), "kinematic", "either dynamic or kinematic"),
    (dict(BOX, dynamic=True, mass=1.0, angular_velocity=[0.0, 1.0]), "angular_velocity", "three finite numbers"),
    (dict(BOX, dynamic=True, mass=1.0, angular_velocity=[0.0, float("inf"), 0.0]), "angular_velocity", "three finite numbers"),
    (dict(SPHERE, mass=1.0), "mass", "only a rigid body takes it"),
    (dict(SPHERE, density=1.0), "density", "only a rigid body takes it"),
    (dict(BOX, angular_velocity=[0, 1, 0]), "angular_velocity", "only a rigid body takes it"),
    (dict(BOX, gravity=False), "gravity", "only a rigid body takes it"),
])
def test_every_refusal_names_entry_and_field(entry, field, text):
    with pytest.raises(ValueError, match=rf"^collider 1: {field}: .*{text}"):
        parse_colliders([dict(type="plane"), entry] if entry["type"] != "mesh" else [dict(type="plane"), entry])


def test_keys_parse_into_the_shape_and_a_body_record():
    cs = parse_colliders([dict(type="plane"), dict(SPHERE, dynamic=True, density=4000.0, velocity=[0, -1, 0], gravity=False),
                          dict(BOX, kinematic=True, angular_velocity=[0, 6, 0], surface="slip"), dict(SPHERE, surface="slip")])
    assert [type(c) for c in cs] == [sc.Plane, Sphere, Box, Sphere] and [c.body is not None for c in cs] == [False, True, True, False]
    s, b = cs[1].body, cs[2].body
    assert isinstance(s, RigidBody) and not s.kinematic and not s.gravity and s.flags == 2 and s.angular_velocity == (0.0, 0.0, 0.0)
    assert b.kinematic and b.gravity and b.flags == 1 and b.mass == 1.0 and b.angular_velocity == (0.0, 6.0, 0.0)
    assert sc.bodies_of(cs) == [(1, s), (2, b)]
    assert not cs[1].moving and cs[1].velocity == (0.0, -1.0, 0.0)      # a body is not advanced by the host
    assert cs[3].body is None and cs[3] == parse_colliders([dict(SPHERE, surface="slip")])[0]
    # mass and density agree
    vol = 4.0 / 3.0 * math.pi * 0.1 ** 3
    assert s.mass == 4000.0 * vol
    by_mass = parse_colliders([dict(SPHERE, dynamic=True, mass=4000.0 * vol)])[0].body
    assert by_mass.mass == s.mass and by_mass.inertia == s.inertia
    bd = parse_colliders([dict(BOX, dynamic=True, density=250.0)])[0].body
    assert abs(bd.mass - 2.0) < 1e-15 * 2.0 * 4      # 250 x (8 x 0.1 x 0.05 x 0.2), a few roundings
    text = sc.describe(cs)
    assert text.count("rigid body: ") == 2 and "rigid body: dynamic mass=" in text and "rigid body: kinematic mass=1 " in text
    assert "gravity=off" in text and "angular_velocity=(0.0, 6.0, 0.0)" in text
    assert sc.describe(cs[:1] + cs[3:]) == sc.describe(parse_colliders([dict(type="plane"), dict(SPHERE, surface="slip")]))
    arr = sc.pack_bodies(cs)
    assert len(arr) == 2 and (arr[0].collider, arr[0].flags, arr[0].mass) == (1, 2, s.mass) and tuple(arr[1].angular_velocity) == (0.0, 6.0, 0.0)
    assert sc.pack_bodies(cs[:1]) is None


def test_inertia_against_the_closed_forms():
    s = parse_colliders([dict(SPHERE, dynamic=True, mass=3.0)])[0]
    assert np.allclose(s.body.inertia, (0.4 * 3.0 * 0.01,) * 3, rtol=4e-16, atol=0) and tuple(xr.inertia(s, 3.0)) == s.body.inertia
    b = parse_colliders([dict(BOX, dynamic=True, mass=6.0)])[0]
    hx, hy, hz = 0.1, 0.05, 0.2
    want = (2.0 * (hy * hy + hz * hz), 2.0 * (hx * hx + hz * hz), 2.0 * (hx * hx + hy * hy))
    assert np.allclose(b.body.inertia, want, rtol=1e-15, atol=0) and np.array_equal(xr.inertia(b, 6.0), b.body.inertia)
    # against a quadrature of the solid box: I_x = rho int (y^2 + z^2) dV
    n = 64
    g = (np.arange(n) + 0.5) / n * 2 - 1
    X, Y, Z = np.meshgrid(g * hx, g * hy, g * hz, indexing="ij")
    dm = 6.0 / n ** 3
    quad = (dm * (Y * Y + Z * Z).sum(), dm * (X * X + Z * Z).sum(), dm * (X * X + Y * Y).sum())
    assert np.allclose(quad, want, rtol=1e-3)


def test_quaternion_and_rotation_agree():
    for angles in ((0, 0, 0), (10, 20, 30), (170, -80, 95), (0, 180, 0), (180, 0, 0), (0, 0, 180), (120, 120, -120)):
        R = np.asarray(sc.euler_xyz_deg_to_rot(angles)).reshape(3, 3)
        q = xr.rot_quat(R)
        assert abs(float(q @ q) - 1.0) < 1e-15 and np.abs(xr.quat_rot(q) - R).max() < 1e-15, angles
    # the exponential: a turn of theta about an axis, in many steps on either side of the series threshold
    axis = np.asarray(rc.W_DIR)
    for steps, rate in ((7, 300.0), (1000, 5.0)):      # theta per step: 0.3 (sin / cos), 5e-3 (series)
        q = np.array([1.0, 0.0, 0.0, 0.0])
        for _ in range(steps):
            q = xr.rotate(q, rate * axis, 1e-3)
        th = steps * rate * 1e-3
        assert np.abs(q - np.concatenate([[math.cos(th / 2)], math.sin(th / 2) * axis])).max() < 1e-13
    one = np.array([1.0, 0.0, 0.0, 0.0])
    for th in (xr.SERIES_BELOW * (1 - 1e-9), xr.SERIES_BELOW * (1 + 1e-9), 1e-5, 1e-9, 0.0):      # the series against sin, both sides
        want = np.concatenate([[math.cos(th / 2)], math.sin(th / 2) * axis])
        assert np.abs(xr.rotate(one, th * axis, 1.0) - want).max() < 2e-16, th


def test_free_body_in_the_twin(capsys):
    """No contact.  With gravity: the centre after n steps is c0 + n v0 dt + g dt^2 n (n + 1) / 2 to fp64 rounding, and |q| = 1 to
    1e-15 after 10^4 steps.  Without: a box with three different inertias keeps Lc bit for bit (it is never touched).  The drift of
    the kinetic energy over 10^4 steps is printed, not bounded: it is a property of the integrator, not of the port."""
    box = parse_colliders([dict(BOX, dynamic=True, mass=2.0, velocity=[0.3, 0.1, -0.2], angular_velocity=[3.0, -7.0, 5.0])])[0]
    assert len(set(box.body.inertia)) == 3
    g, dt, n = np.array([0.0, -9.8, 0.0]), 1e-3, 10000
    s0 = xr.initial_state(box, fp32=False)
    s = s0
    for _ in range(n):
        s = xr.rigid_step(s, None, box.body, dt, g)
    want = rc.free_fall_centre(s0.c, s0.P / 2.0, g, dt, n)
    assert np.abs(s.c - want).max() < 1e-12 * np.abs(want).max()         # 10^4 additions of ~1e-3: rounding grows like n ulp
    assert abs(math.sqrt(float(s.q @ s.q)) - 1.0) < 1e-15
    assert np.array_equal(s.Lc, s0.Lc)                                     # gravity has no torque about the centre
    body0 = box.body.__class__(**dict(box.body.__dict__, gravity=False))
    f, e0 = s0, xr.kinetic_energy(s0, body0)
    for _ in range(n):
        f = xr.rigid_step(f, None, body0, dt, g)
    assert np.array_equal(f.Lc, s0.Lc) and np.array_equal(f.P, s0.P)
    assert abs(math.sqrt(float(f.q @ f.q)) - 1.0) < 1e-15
    assert np.abs(f.c - (s0.c + n * dt * s0.P / 2.0)).max() < 1e-12
    drift = xr.kinetic_energy(f, body0) / e0 - 1.0
    with capsys.disabled():
        print(f"\nfree box, 10^4 steps of dt = 1e-3, |w| = {np.linalg.norm(xr.velocities(s0, body0)[1]):.3g}: kinetic energy drift {drift:+.3e} (relative)")
    assert math.isfinite(drift)
    # a kinematic body keeps v and w whatever row it is handed
    kin = parse_colliders([dict(BOX, kinematic=True, velocity=[0.3, 0.1, -0.2], angular_velocity=[3.0, -7.0, 5.0])])[0]
    k0 = xr.initial_state(kin, fp32=False)
    k = xr.rigid_step(k0, np.arange(1.0, 10.0), kin.body, dt, g)
    assert np.array_equal(k.P, k0.P) and np.array_equal(k.Lc, k0.Lc) and np.array_equal(k.c, k0.c + np.array([0.3, 0.1, -0.2]) * dt)
    assert np.array_equal(xr.velocities(k, kin.body)[1], [3.0, -7.0, 5.0])


def test_a_row_moves_the_body_as_the_definition_says():
    s = parse_colliders([dict(SPHERE, dynamic=True, mass=4.0, velocity=[0.1, 0.0, 0.0])])[0]
    s0 = xr.initial_state(s, fp32=False)
    J, r = np.array([0.0, 2.0, 0.0]), np.array([0.05, 0.0, 0.0])            # an impulse at c + r
    row = np.concatenate([J, np.cross(s0.c + r, J), [0.0, 1.0, 1.0]])
    n = xr.rigid_step(s0, row, s.body, 0.5, np.zeros(3))
    assert np.allclose(n.P, s0.P + J) and np.allclose(n.Lc, np.cross(r, J), atol=1e-16)
    assert np.allclose(n.c, s0.c + 0.5 * (s0.P + J) / 4.0)
    v, w = xr.velocities(n, s.body)
    assert np.allclose(w, np.cross(r, J) / s.body.inertia[0])
    assert np.allclose(xr.body_velocity(n.c, v, w, n.c + r), v + np.cross(w, r))
    pc, pw = xr.posed(s, n)
    assert pc.center == tuple(n.c) and pc.velocity == tuple(v) and np.array_equal(pw, w) and pc.body is s.body


@pytest.mark.parametrize("shape", ["plane", "sphere", "box"])
@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
def test_default_paths_return_the_bits_they_returned(shape, surface):
    """apply_collider(..., omega=None) against the function as it was (restated here from its definition), and contact_rows with
    and without the new keyword, on the existing collider cases"""
    G = 16
    _, _, _, (gmv, gm, gv) = _case(3001, G, "noslip")
    c = parse_colliders([collider_cfg(shape, surface, G)])[0]
    p, u = xc.node_positions(G), gv.reshape(-1, 3)
    sdf, n = xc.sdf_normal(c, p)
    vc = torch.as_tensor(c.velocity, dtype=u.dtype).expand_as(u)
    if surface == "sticky":
        new = vc
    else:
        w = u - vc
        vn = (w * n).sum(-1, keepdim=True)
        if surface == "slip":
            hit = u - vn * n
        else:
            vt = w - vn * n
            s2 = (vt * vt).sum(-1, keepdim=True)
            s = torch.where(s2 > 0, s2, torch.ones_like(s2)).sqrt()
            hit = vc + torch.where(s2 > 0, torch.clamp(1.0 + float(c.friction) * vn / s, min=0.0) * vt, torch.zeros_like(vt))
        new = torch.where(vn < 0, hit, u)
    was = torch.where((sdf < 0)[:, None], new, u)
    assert torch.equal(xc.apply_collider(c, p, u), was) and torch.equal(xc.apply_collider(c, p, u, omega=None), was)
    assert torch.equal(xc.apply_colliders([c], gv, G), was.reshape(gv.shape))
    assert torch.equal(xc.apply_colliders([c], gv, G, omegas=[None]), was.reshape(gv.shape))
    const = _case(3001, G, "noslip")[0]
    a = xk.contact_rows(gmv, gm, colliders=[c], **cc.const_kwargs(const))
    b = xk.contact_rows(gmv, gm, colliders=[c], omegas=[None], **cc.const_kwargs(const))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], cc.twin(const, gmv, gm, [c])[0])
    if shape != "plane":      # and a zero angular velocity is the constant velocity (w x d = 0 exactly)
        assert torch.equal(xc.apply_collider(c, p, u, omega=(0.0, 0.0, 0.0)), was)


def test_the_cases_of_the_gpu_tests_hold_their_margins():
    for N, G in rc.SIZES:
        for shape in rc.SHAPES:
            cs = rc.bodies([rc.body_cfg(shape, "friction", G)], G)
            w = np.asarray(cs[0].body.angular_velocity)
            assert np.linalg.norm(w) > 0 and np.allclose(w / np.linalg.norm(w), rc.W_DIR)
            assert int(rc.inside(cs[0], G).sum()) >= 8
        assert [type(c).__name__ for c in rc.chain_pair(G)] == ["Box", "Sphere"]
        sph = dict(collider_cfg("sphere", "slip", G), dynamic=True, mass=rc.MASS, angular_velocity=list(rc.omega_for(cc.pair(G)[1], G)))
        assert len(rc.bodies([collider_cfg("plane", "friction", G), sph], G)) == 2
    pad = cc.padding_sphere("friction")[0]
    assert rc.bodies([dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.15, surface="friction", friction=0.4, dynamic=True, mass=rc.MASS,
                           angular_velocity=list(rc.omega_for(pad, 10)))], 10)[0].body is not None


class _LogModel(object):
    """what RigidLog reads of a model: constant.dt, the bodies, and per step rigid_rows() / rigid_state()"""

    def __init__(self, colliders, masses):
        self.constant = type("K", (), dict(dt=1e-3))()
        self.prescribed_colliders = list(colliders)
        self.rigid_bodies = sc.bodies_of(colliders)
        self._masses, self._k = masses, 0

    def rigid_rows(self):
        rows = torch.zeros(1 + len(self.prescribed_colliders), 9, dtype=torch.float64)
        rows[:, 7] = torch.as_tensor(self._masses[self._k], dtype=torch.float64)
        return rows

    def rigid_state(self):
        self._k += 1
        out = torch.zeros(len(self.rigid_bodies), 19, dtype=torch.float64)
        out[:, 3] = 1.0
        out[:, 1] = 0.5 - 0.01 * self._k
        return out


def test_the_log_writes_its_csv_and_names_the_frame_of_the_peak_mass_ratio(tmp_path):
    import csv
    from neuma_amd.rigid import CSV_COLUMNS, RigidLog
    cs = parse_colliders([dict(type="plane"), dict(SPHERE, dynamic=True, mass=2.0), dict(BOX, dynamic=True, mass=4.0),
                          dict(BOX, kinematic=True)])
    # per step: the mass column of the rows [walls, plane, sphere, box, kinematic box]
    masses = [[9.0, 9.0, 0.5, 1.0, 50.0], [9.0, 9.0, 3.0, 4.0, 50.0], [9.0, 9.0, 5.0, 3.9, 50.0], [9.0, 9.0, 1.0, 0.0, 50.0]]
    log = RigidLog(_LogModel(cs, masses))
    assert log.names == ["1:sphere", "2:box", "3:box"]
    assert log.mass_ratio_notes() == []
    for _ in masses:
        log.after_step()
    notes = log.mass_ratio_notes()
    assert len(notes) == 1                                  # the box peaks at exactly 1 (not beyond), the kinematic body is not moved
    assert notes[0].startswith("rigid body 1:sphere: peak contact mass / M = 2.5 at frame 3 ") and "diverges beyond 2" in notes[0]
    over = RigidLog(_LogModel(cs[:2], [[9.0, 9.0, 2.0], [9.0, 9.0, 3.0], [9.0, 9.0, 0.1]]))
    for _ in range(3):
        over.after_step()
    assert over.mass_ratio_notes() == ["rigid body 1:sphere: peak contact mass / M = 1.5 at frame 2 (> 1: the explicit coupling "
                                       "overshoots; use a heavier body or a smaller dt)"]
    lines = list(csv.reader(open(log.write_csv(tmp_path / "rigid_x.csv"))))
    assert tuple(lines[0]) == CSV_COLUMNS and len(lines) == 1 + 4 * 3
    assert lines[1][:3] == ["1", repr(1e-3), "1:sphere"] and lines[-1][:3] == ["4", repr(4 * 1e-3), "3:box"]
    assert float(lines[1][4]) == 0.49 and float(lines[-1][4]) == 0.46 and float(lines[1][6]) == 1.0
