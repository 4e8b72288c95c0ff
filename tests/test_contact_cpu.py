"""CPU: the contact report's fp64 definition (neuma_amd/extras/contact.py) - its momentum identity against the oracle's p2g / g2p
and the exact consequences of each surface law -, the arithmetic of ContactMeter, the flag of both entry points and the
host-only refusals of nm_mpm_contact.  Cases: tests/contact_cases.py."""
import csv
import ctypes as C
import types

import pytest
import torch

import contact_cases as cc
from contact_cases import MU, SIZES, BCS
from oracle import mpm as om
from neuma_amd.extras import colliders as xc
from neuma_amd.extras import contact as xk
from neuma_amd.sim.colliders import Plane, Sphere, parse_colliders
from test_gpu_colliders import _case, collider_cfg


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
def test_momentum_identity_of_the_definition(N, G, bc):
    """oracle p2g -> the twin's chain -> oracle g2p: the momentum the particles get back is what the free grid held minus what the
    rows hand to the walls and the colliders.  Bound: 1e-12 x sum m_p |v_p'| (fp64 sums of < 1e5 terms; measured <= 9e-16 x 22)."""
    const, (vol, rho, clip, en), ins, (gmv, gm, gv) = _case(N, G, bc)
    cs = cc.pair(G)
    assert cc.nodes_in_both(cs, gm, G) >= 8, "the chain order does not matter in this case"      # 129 (G = 32), 15 (G = 16)
    chain = xk.contact_chain(gmv, gm, colliders=cs, **cc.const_kwargs(const))
    assert torch.equal(chain[1].reshape(G, G, G, 3), gv)            # the twin's box boundary condition is the oracle's grid_op
    rows, scale = cc.twin(const, gmv, gm, cs)
    assert rows.shape == (3, 9) and scale.shape == (3,) and rows.dtype == torch.float64
    _, ov, _, _ = om.g2p(const, clip, en, ins[0], ins[3], chain[-1].reshape(G, G, G, 3), ins[1], ins[2])
    free = (gm.reshape(-1, 1) * chain[0]).sum(0)
    residual = cc.momentum(vol, rho, en, ov) - (free - rows[:, xk.J].sum(0))
    mp = (vol * rho)[en != 0]
    size = float((mp * ov[en != 0].norm(dim=-1)).sum())
    print(f"momentum identity N={N} G={G} {bc}: residual {float(residual.abs().max()):.3e} scale {size:.3e}")
    assert float(residual.abs().max()) <= 1e-12 * size
    assert float(rows[0, xk.J].abs().max()) > 0 and float(rows[0, xk.N]) == 0.0      # near_wall: the walls row is not empty
    assert all(float(rows[r, xk.NODES]) >= 8 for r in range(3))


@pytest.mark.parametrize("N,G", SIZES)
def test_consequences_of_the_surface_laws(N, G):
    const, _, _, (gmv, gm, gv) = _case(N, G, "freeslip")
    p = xc.node_positions(G)
    # slip plane: the impulse is along the normal, and N is its size
    cs = parse_colliders([collider_cfg("plane", "slip", G)])
    rows, _ = cc.twin(const, gmv, gm, cs)
    n = torch.tensor(cs[0].normal, dtype=torch.float64)
    Jv = rows[1, xk.J]
    assert float((Jv - (Jv @ n) * n).norm()) <= 1e-13 * float(Jv.norm()) and float(Jv.norm()) > 0
    assert abs(float(rows[1, xk.N]) + float(Jv @ n)) <= 1e-13 * float(Jv.norm()) and float(rows[1, xk.N]) > 0
    # friction plane: the tangential impulse stays inside the Coulomb cone of the normal one
    cs = parse_colliders([collider_cfg("plane", "friction", G)])
    rows, _ = cc.twin(const, gmv, gm, cs)
    Jv = rows[1, xk.J]
    tangential = float((Jv - (Jv @ n) * n).norm())
    print(f"friction plane G={G}: |J_t| {tangential:.4g} mu N {MU * float(rows[1, xk.N]):.4g}")      # 0.055 / 0.454, 0.087 / 1.25
    assert tangential <= MU * float(rows[1, xk.N])
    # sticky sphere at rest: the body loses all the momentum it had inside
    cs = parse_colliders([collider_cfg("sphere", "sticky", G, velocity=(0.0, 0.0, 0.0))])
    rows, _ = cc.twin(const, gmv, gm, cs)
    inside = (xc.sdf_normal(cs[0], p)[0] < 0) & (gm.reshape(-1) > 0)
    held = (gm.reshape(-1, 1) * gv.reshape(-1, 3))[inside]
    assert torch.allclose(rows[1, xk.J], held.sum(0), rtol=1e-13, atol=0)
    assert torch.allclose(rows[1, xk.L], torch.linalg.cross(p[inside], held).sum(0), rtol=1e-12, atol=1e-15)
    assert float(rows[1, xk.NODES]) == float(inside.sum()) and abs(float(rows[1, xk.MASS]) - float(gm.reshape(-1)[inside].sum())) < 1e-15
    # no colliders: the walls row alone
    rows, scale = cc.twin(const, gmv, gm, [])
    assert rows.shape == (1, 9) and scale.shape == (1,)
    lo, hi = xk.boundary_layer(G, const.bound)
    layer = (lo | hi).any(-1) & (gm.reshape(-1) > 0)
    assert float(rows[0, xk.NODES]) == float(layer.sum()) > 0 and float(rows[0, xk.N]) == 0.0


def test_geometry_margins_hold_for_every_case_used():
    """what tests/test_gpu_contact.py relies on, asserted in fp64 where no GPU is needed"""
    for N, G in SIZES:
        for shape in cc.SHAPES:
            cc.single(shape, "slip", G)
        cc.pair(G)
        for bc in BCS:
            cc.analytic_and_field(N, G, bc)
    const, _, ins = cc.padding_case()
    for surface in ("sticky", "friction"):
        cs = cc.padding_sphere(surface)
        assert int((xc.sdf_normal(cs[0], xc.node_positions(10))[0] < 0).sum()) == 19


class _FakeModel(object):
    """what ContactMeter reads of a model: constant.dt, the collider lists, contact(), step_colliders()"""

    def __init__(self, colliders, reports):
        self.constant = types.SimpleNamespace(dt=2e-3)
        self.colliders, self.field_colliders = list(colliders), []
        self._reports = list(reports)

    def contact(self):
        from neuma_amd.sim.mpm import ContactReport
        return ContactReport(self._reports.pop(0), ["walls"] + [f"{i}:{type(c).__name__.lower()}" for i, c in enumerate(self.colliders)])

    def step_colliders(self):
        self.colliders = [c.advanced(self.constant.dt) if c.moving else c for c in self.colliders]


def test_contact_meter_arithmetic(tmp_path):
    from neuma_amd.contact import CSV_COLUMNS, ContactMeter, reference_points
    from neuma_amd.sim.mpm import ContactReport
    g = torch.Generator().manual_seed(3)
    reports = [torch.randn(3, 9, generator=g, dtype=torch.float64) for _ in range(3)]
    cs = [Plane(point=(0.1, 0.2, 0.3), normal=(0.0, 1.0, 0.0)), Sphere(center=(0.5, 0.4, 0.6), radius=0.1, velocity=(0.0, 50.0, 0.0))]
    model = _FakeModel(cs, reports)
    meter = ContactMeter(model)
    dt = 2e-3
    # the torque shift of a report
    rep = ContactReport(reports[0], ["walls", "0:plane", "1:sphere"])
    r0 = torch.tensor([0.5, 0.4, 0.6], dtype=torch.float64)
    want = (reports[0][:, 3:6] - torch.linalg.cross(r0.expand(3, 3), reports[0][:, 0:3])) / dt
    assert torch.equal(rep.torque(dt, r0), want) and torch.equal(rep.force(dt), reports[0][:, 0:3] / dt)
    assert torch.equal(rep.torque(dt, r0), xk.torque(reports[0], dt, r0)) and torch.equal(rep.force(dt), xk.force(reports[0], dt))
    assert torch.equal(rep.normal, reports[0][:, 6]) and torch.equal(rep.mass, reports[0][:, 7]) and torch.equal(rep.nodes, reports[0][:, 8])
    # frame 1: two substeps, the sphere moves between them and the reference is where it was when each substep was recorded
    refs = []
    for _ in range(2):
        refs.append(torch.tensor(reference_points(model), dtype=torch.float64))
        meter.record()
        model.step_colliders()
    assert refs[0][0].tolist() == [0.0, 0.0, 0.0] and refs[0][1].tolist() == [0.1, 0.2, 0.3] and refs[0][2].tolist() == [0.5, 0.4, 0.6]
    assert refs[1][2].tolist() == [0.5, 0.4 + dt * 50.0, 0.6] and refs[1][1].tolist() == [0.1, 0.2, 0.3]
    summed = meter.frame()
    assert torch.equal(summed.rows, reports[0] + reports[1]) and summed.names == ["walls", "0:plane", "1:sphere"]
    # frame 2: one substep
    meter.record()
    meter.frame()
    with pytest.raises(ValueError, match="contact:"):
        meter.frame()
    path = meter.write_csv(tmp_path / "contacts.csv")
    lines = list(csv.reader(open(path)))
    assert tuple(lines[0]) == CSV_COLUMNS == ("frame", "time", "row", "name", "Fx", "Fy", "Fz", "Tx", "Ty", "Tz", "normal", "mass", "nodes")
    assert len(lines) == 1 + 2 * 3
    body = {(int(l[0]), int(l[2])): l for l in lines[1:]}
    tq = sum(reports[s][:, 3:6] - torch.linalg.cross(refs[s], reports[s][:, 0:3]) for s in range(2))
    for r in range(3):
        line = body[1, r]
        assert float(line[1]) == 2 * dt and line[3] == summed.names[r]
        got = torch.tensor([float(a) for a in line[4:]], dtype=torch.float64)
        assert torch.allclose(got[0:3], summed.rows[r, 0:3] / (2 * dt), rtol=1e-15, atol=0)
        assert torch.allclose(got[3:6], tq[r] / (2 * dt), rtol=1e-14, atol=0)
        assert torch.allclose(got[6:9], torch.stack([summed.rows[r, 6] / (2 * dt), summed.rows[r, 7] / 2, summed.rows[r, 8] / 2]), rtol=1e-15, atol=0)
    assert float(body[2, 0][1]) == pytest.approx(3 * dt, rel=1e-15)
    said = meter.summary()
    assert said.startswith("contacts: 2 frames") and all(name + ": peak |F| = " in said for name in summed.names) and "total impulse" in said
    k = 1 + int((reports[2][2, 0:3] / dt).norm() > (summed.rows[2, 0:3] / (2 * dt)).norm())
    assert f"1:sphere: peak |F| = {float(max((reports[2][2, 0:3] / dt).norm(), (summed.rows[2, 0:3] / (2 * dt)).norm())):.6g} at frame {k}" in said


def test_flag_and_config_key_are_parsed_by_both_entry_points():
    from neuma_amd import contact, evaluate, inference
    for mod in (evaluate, inference):
        base = ["-c", "x.yaml", "-vn", "v"]
        assert mod.parse_args(base).report_contacts is False
        assert mod.parse_args(base + ["--report_contacts"]).report_contacts is True
    assert contact.wanted({"report_contacts": True}, {}) and contact.wanted({"report_contacts": False}, {"report_contacts": True})
    assert not contact.wanted({"report_contacts": False}, {"colliders": []}) and not contact.wanted({}, None)


def test_null_arguments_are_refused_on_the_host():
    from neuma_amd import _lib as L
    lib = L.lib()
    buf = (C.c_double * 9)()
    assert lib.nm_mpm_contact(None, C.cast(buf, C.c_void_p), None) == -1
    assert b"contact:" in lib.nm_last_error() and b"null handle" in lib.nm_last_error()
    fake = C.c_void_p(0x1000)        # never dereferenced: rows is checked before the handle is used
    assert lib.nm_mpm_contact(fake, None, None) == -1
    assert b"contact:" in lib.nm_last_error() and b"null rows" in lib.nm_last_error()
