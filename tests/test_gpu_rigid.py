"""GPU: rigid bodies of the per-operator MPM path (csrc/nm_rigid.h, k_rigid_step; the body variants k_grid_collide_rigid /
k_contact_rows_rigid; MPMModel.step_colliders() / rigid_state()) against the fp64 definition neuma_amd/extras/rigid.py and the
twins that gained the body's velocity field (extras/colliders.py, extras/contact.py), all FED THE GPU'S OWN exported grid, rows
and states - which isolates the new code from the scatter in front of it and keeps chaotic divergence out of chained steps.
Cases and their fp64 margins: tests/rigid_cases.py.

Bounds.  Node velocities: contact_cases.BOUND (7e-7, mass-weighted), the bound these very colliders hold at w = 0; the body's
velocity field adds three fp32 roundings of a term that is at most |VC| (rigid_cases.omega_for), i.e. < 2e-8 absolute against
velocities of order 1.  The step: 1e-12 relative, fp64 against fp64.  Momentum: the bound of
test_gpu_contact.test_momentum_identity_on_the_device; the body's update is exact in fp64 and adds nothing to it."""
import csv
import ctypes as C
import math

import numpy as np
import pytest
import torch

import contact_cases as cc
import rigid_cases as rc
from gpu_util import dev, build_model, build_statics, measured, mpm_case, parity, rel_max
from neuma_amd.extras import contact as xk
from neuma_amd.extras import rigid as xr
from rigid_cases import BCS, BOUND, REL, SHAPES, SIZES, SURFACES
from test_gpu_colliders import VC, _case, collider_cfg

pytestmark = pytest.mark.gpu

NAMES = ("x", "v", "C", "F", "stress")


def _model(const, colliders):
    model = build_model(const, dev())
    model.set_colliders(colliders)
    return model


def _state(model, ins):
    state = model.state(ins[0].shape[0])
    state.from_torch(**{k: t.float().to(dev()) for k, t in zip(NAMES, ins)})
    return state


def _setup(N, G, bc, cs):
    const, (vol, rho, clip, en), ins, _ = _case(N, G, bc)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    return const, model, st, (vol, rho, en), ins


def _check_step(case, const, cs, s0, rows, s1):
    """the device states after a step (s1) against rigid_step fed the device's states before (s0) and the device's rows"""
    dt, g = rc.device_dt_gravity(const)
    for k, (idx, body) in enumerate([(i, c.body) for i, c in enumerate(cs) if c.body is not None]):
        want = xr.rigid_step(xr.RigidState.from_row(s0[k]), rows[1 + idx], body, dt, g)
        got = xr.RigidState.from_row(s1[k])
        for name in ("c", "q", "P", "Lc"):
            parity(case, f"body {idx} {name} (rel)", rc.rel(getattr(got, name), getattr(want, name)), REL)
        v, w = xr.velocities(want, body)
        parity(case, f"body {idx} v (rel)", rc.rel(s1[k][13:16], v), REL)
        parity(case, f"body {idx} w (rel)", rc.rel(s1[k][16:19], w), REL)
        assert abs(float(np.linalg.norm(s1[k][3:7])) - 1.0) < 1e-15


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("shape", SHAPES)
def test_response_with_rotation(shape, surface, N, G, bc):
    """One substep against one turning body: every node velocity of the exported grid against the twin on the exported {mv, m}."""
    cs = rc.bodies([rc.body_cfg(shape, surface, G)], G)
    const, model, st, _, ins = _setup(N, G, bc, cs)
    cur = _state(model, ins)
    model.forward(st, cur, model.state(N))
    s0 = model.rigid_state().cpu().numpy()
    assert np.array_equal(s0[0][0:3], np.asarray(cs[0].center, dtype=np.float32).astype(np.float64))      # the pose it was given
    mv, m, vg = model.grid_export()
    want = rc.twin_velocity(const, mv, m, cs, s0)
    plain = xk.contact_chain(mv, m, colliders=[rc.posed_list(cs, s0)[0][0]], **cc.const_kwargs(const))[-1]
    m64 = m.cpu().double().reshape(-1, 1)
    if (shape, surface) != ("sphere", "slip"):      # (a sphere turning about its centre moves along its surface: slip does not see it)
        assert int((((want - plain).abs().max(-1).values > 1e-3) & (m64[:, 0] > 0)).sum()) >= 4, "the rotation moves (almost) no node with mass"
    case = f"rigid {shape}/{surface} N={N} G={G} {bc}: node velocities vs fp64 definition on the exported grid"
    parity(case, "grid v (mass-weighted)", rel_max(vg.reshape(-1, 3) * m.reshape(-1, 1), want * m64), BOUND)
    empty = m64[:, 0] == 0      # nodes no particle touches: the dense export collides them too
    assert float((vg.cpu().double().reshape(-1, 3)[empty] - want[empty]).abs().max()) < 1e-7
    # and the body's contact row against the twin's
    rows = model.contact().rows.cpu()
    ref, scale = rc.twin_rows(const, mv, m, cs, s0)
    S = float(scale[1])
    assert S > 0 and float(rows[1, xk.NODES]) == float(ref[1, xk.NODES]) > 0
    parity(case, "body row J / S", float((rows[1, xk.J] - ref[1, xk.J]).abs().max()) / S, BOUND)
    parity(case, "body row L / (sqrt3 S)", float((rows[1, xk.L] - ref[1, xk.L]).abs().max()) / (math.sqrt(3.0) * S), BOUND)


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_step_against_the_twin_fed_the_devices_rows(shape, N, G, bc):
    cs = rc.bodies([rc.body_cfg(shape, "friction", G)], G)
    const, model, st, _, ins = _setup(N, G, bc, cs)
    model.forward(st, _state(model, ins), model.state(N))
    s0 = model.rigid_state().cpu().numpy()
    rows = model.contact().rows.cpu().numpy()
    model.step_colliders()
    s1 = model.rigid_state().cpu().numpy()
    assert float(np.abs(rows[1, 0:3]).max()) > 0 and rows[1, 8] > 0
    assert not np.array_equal(s0[0][7:13], s1[0][7:13])
    _check_step(f"rigid step {shape}/friction N={N} G={G} {bc} vs fp64 definition on the device's rows", const, cs, s0, rows, s1)
    # the pose the next forward collides against is the new one: the exported grid of one more substep holds the twin at s1.
    # The sphere of these cases starts with its centre ON a grid node (the +x branch of the normal); after the step that node is
    # ~5e-5 from the centre, and its normal d / |d| carries the fp32 rounding of the centre (3e-8) divided by |d| - 6e-4, measured
    # as 4.3e-5 of the largest node momentum.  Which way a node at the very centre of a ball is pushed means nothing; the node is
    # left out of this comparison (and only of this one), every other node is held to the bound.
    cur = _state(model, ins)
    model.forward(st, cur, model.state(N))
    mv, m, vg = model.grid_export()
    want = rc.twin_velocity(const, mv, m, cs, s1)
    keep = torch.ones(G ** 3, 1, dtype=torch.float64)
    if shape == "sphere":
        near = (xk.xc.node_positions(G) - torch.as_tensor(s1[0][0:3])).norm(dim=-1) < 0.25 / G
        assert int(near.sum()) == 1
        keep[near] = 0.0
    parity(f"rigid {shape}/friction N={N} G={G} {bc}: node velocities after a step", "grid v (mass-weighted)",
           rel_max(vg.cpu().double().reshape(-1, 3) * m.cpu().double().reshape(-1, 1) * keep, want * m.cpu().double().reshape(-1, 1) * keep), BOUND)


def _chain(model, st, state, cs, const, steps, case=None):
    """`steps` in-place substeps; per step the device's (state before, rows, state after), checked against the twin if `case`"""
    from neuma_amd.sim import MPMForwardSim
    sim, log = MPMForwardSim(model), []
    for k in range(steps):
        s0 = model.rigid_state()
        outs = sim(st, state)
        rows = model.contact().rows
        model.step_colliders()
        log.append((s0, rows, model.rigid_state()))
    if case is not None:
        for k, (s0, rows, s1) in enumerate(log):
            _check_step(f"{case}, substep {k + 1}", const, cs, s0.cpu().numpy(), rows.cpu().numpy(), s1.cpu().numpy())
    return outs, log


@pytest.mark.parametrize("N,G", SIZES)
def test_eight_chained_substeps(N, G):
    """a dynamic box and a dynamic sphere side by side (list order: the box first), the twin re-seeded from the device each step"""
    cs = rc.chain_pair(G)
    const, model, st, _, ins = _setup(N, G, "noslip", cs)
    _, log = _chain(model, st, _state(model, ins), cs, const, 8, f"rigid chain box + sphere N={N} G={G}")
    assert all(float(r[1:, 8].min()) > 0 for _, r, _ in log), "a body lost contact"
    assert not torch.equal(log[0][2], log[7][2])


def test_padding_lanes():
    """G = 10: 3 blocks of 4 nodes per axis, padding lanes in every edge block (contact_cases.padding_case)"""
    const, (vol, rho, clip, en), ins = cc.padding_case()
    node = dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.15, surface="friction", friction=0.4, velocity=list(VC), dynamic=True,
                mass=rc.MASS)
    cs = rc.bodies([dict(node, angular_velocity=list(rc.omega_for(cc.padding_sphere("friction")[0], 10)))], 10)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    _, log = _chain(model, st, _state(model, ins), cs, const, 2, "rigid sphere/friction N=1000 G=10 (padding lanes)")
    assert float(log[0][1][1, 8]) == 19.0
    mv, m, _ = model.grid_export()      # the grid of the second substep, collided at the pose after the first
    ref, scale = rc.twin_rows(const, mv, m, cs, log[1][0].cpu().numpy())
    rows = log[1][1].cpu()
    parity("rigid sphere/friction N=1000 G=10 (padding lanes): rows vs fp64 definition", "body row J / S",
           float((rows[1, xk.J] - ref[1, xk.J]).abs().max()) / float(scale[1]), BOUND)
    assert float(rows[1, xk.NODES]) == float(ref[1, xk.NODES])


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("N,G", SIZES)
def test_momentum_with_a_body(N, G, bc):
    """Linear and angular momentum of particles plus body across one substep with gravity on, [plane / friction, sphere / slip] with
    the sphere a dynamic body:  sum m_p v_p' + P' = sum m_i u_free,i - sum_{r != body} J_r + P + M g dt, and about the origin
    sum m_p (x_p x v_p' + dx^2/4 axial(C_p')) + Lc' + c' x P' = sum m_i p_i x u_free,i - sum_{r != body} L_r + Lc + c x P + c x M g dt
    (x_p the position the particle gathered at; the affine term is what the quadratic B-spline's second moment dx^2/4 leaves of
    sum_i w_ip (p_i - x_p) x u_i).  Both residuals are held to one bound, that of
    test_gpu_contact.test_momentum_identity_on_the_device: BOUND max|v'| sum m_p + BOUND sum_r S_r."""
    const, (vol, rho, clip, en), ins, _ = _case(N, G, bc)
    sph = dict(collider_cfg("sphere", "slip", G), dynamic=True, mass=rc.MASS, angular_velocity=None)
    sph["angular_velocity"] = list(rc.omega_for(cc.pair(G)[1], G))
    cs = rc.bodies([collider_cfg("plane", "friction", G), sph], G)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    cur, nxt = _state(model, ins), model.state(N)
    model.forward(st, cur, nxt)
    _, v_next, C_next, _, _ = [t.cpu().double() for t in nxt.to_torch()]
    s0 = model.rigid_state().cpu().numpy()[0]
    rows = model.contact().rows.cpu()
    model.step_colliders()
    s1 = model.rigid_state().cpu().numpy()[0]
    mv, m, _ = model.grid_export()
    _, scale = rc.twin_rows(const, mv, m, cs, s0[None])
    dt, g = rc.device_dt_gravity(const)
    m64 = m.cpu().double().reshape(-1)
    p = xk.xc.node_positions(G)
    free = m64[:, None] * xk.free_velocity(mv.cpu().double().reshape(-1, 3), m64, const.dt, const.gravity, const.eps)
    mp = (vol.float() * rho.float()).double()
    e = en != 0
    x_old = ins[0][e]
    body = cs[1].body
    c0, P0, L0, c1, P1, L1 = (rc.tensor(a) for a in (s0[0:3], s0[7:10], s0[10:13], s1[0:3], s1[7:10], s1[10:13]))
    Mg = rc.tensor(body.mass * g * dt)
    got = (mp[:, None] * v_next)[e].sum(0) + P1
    want = free.sum(0) - rows[0, xk.J] - rows[1, xk.J] + P0 + Mg
    lin_bound = BOUND * float(v_next.abs().max()) * float(mp[e].sum()) + BOUND * float(scale.sum())
    case = f"rigid momentum N={N} G={G} {bc}"
    parity(case, "linear residual (abs)", float((got - want).abs().max()), lin_bound)
    Cn = C_next[e]
    axial = torch.stack([Cn[:, 2, 1] - Cn[:, 1, 2], Cn[:, 0, 2] - Cn[:, 2, 0], Cn[:, 1, 0] - Cn[:, 0, 1]], dim=-1)
    got_a = (mp[e][:, None] * (torch.linalg.cross(x_old, v_next[e]) + (const.dx ** 2 / 4.0) * axial)).sum(0) + L1 + torch.linalg.cross(c1, P1)
    want_a = torch.linalg.cross(p, free).sum(0) - rows[0, xk.L] - rows[1, xk.L] + L0 + torch.linalg.cross(c0, P0) + torch.linalg.cross(c0, Mg)
    parity(case, "angular residual about the origin (abs)", float((got_a - want_a).abs().max()), lin_bound)
    assert float(rows[2, xk.NODES]) > 0 and float(rows[2, xk.J].abs().max()) > 0      # the body took part


@pytest.mark.parametrize("shape", SHAPES)
def test_kinematic_body_keeps_its_velocities(shape):
    N, G = 3001, 16
    cs = rc.bodies([rc.body_cfg(shape, "friction", G, kind="kinematic")], G)
    const, model, st, _, ins = _setup(N, G, "noslip", cs)
    state = _state(model, ins)
    _, log = _chain(model, st, state, cs, const, 3, f"kinematic {shape} N={N} G={G}")
    dt, _ = rc.device_dt_gravity(const)
    first = log[0][0].cpu().numpy()[0]
    w = np.asarray(cs[0].body.angular_velocity)
    q = first[3:7].copy()
    for k, (s0, rows, s1) in enumerate(log, start=1):
        assert float(rows[1, 8]) > 0 and float(rows[1, 0:3].abs().max()) > 0               # a non-zero contact row ...
        assert torch.equal(s0[:, 7:13], s1[:, 7:13]) and torch.equal(s1[:, 13:19], log[0][0][:, 13:19])      # ... leaves P, Lc, v, w alone
        q = xr.rotate(q, w, dt)
        got = s1.cpu().numpy()[0]
        parity(f"kinematic {shape} N={N} G={G}, substep {k}", "c vs c0 + k v dt (rel)", rc.rel(got[0:3], first[0:3] + k * dt * first[13:16]), REL)
        parity(f"kinematic {shape} N={N} G={G}, substep {k}", "q vs exp(w dt / 2)^k q0 (rel)", rc.rel(got[3:7], q), REL)
    assert np.array_equal(first[16:19], w) and np.array_equal(first[13:16], np.asarray(VC, dtype=np.float32).astype(np.float64))


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_law_with_pose_arguments_is_the_law(shape, surface):
    """nm_collide.h spells collide_normal / collide_apply twice (as they were, and with pose and v_c as arguments).  A kinematic body
    with w = 0 runs the second pair on the very pose and velocity the first pair reads from the collider: the grids of the two must
    agree to the project's bound for these cases - and, past it, the rows of their contact reports."""
    N, G = 3001, 16
    plain = rc.bodies([collider_cfg(shape, surface, G)], G)
    body = rc.bodies([rc.body_cfg(shape, surface, G, kind="kinematic", omega=(0.0, 0.0, 0.0))], G)
    got = []
    for cs in (plain, body):
        const, model, st, _, ins = _setup(N, G, "noslip", cs)
        model.forward(st, _state(model, ins), model.state(N))
        mv, m, vg = model.grid_export()
        got.append((mv, m, vg, model.contact().rows.cpu()))
    (mv0, m0, v0, r0), (mv1, m1, v1, r1) = got
    assert torch.equal(m0, m1) or rel_max(m1, m0) < 1e-6       # (the scatters' float atomics: the two grids are two runs)
    case = f"rigid law with pose arguments {shape}/{surface} N={N} G={G} against the plain kernels"
    parity(case, "grid v (mass-weighted)", rel_max(v1 * m1[..., None], v0 * m0[..., None]), BOUND)
    S = float(rc.twin_rows(const, mv0, m0, plain, [])[1][1])
    parity(case, "row J / S", float((r1[1, xk.J] - r0[1, xk.J]).abs().max()) / S, BOUND)
    assert float(r1[1, xk.NODES]) == float(r0[1, xk.NODES]) > 0


def _kernels(run):
    """names of the kernels the library launched inside run() (nm_prof_report)"""
    from neuma_amd import _lib as L
    lib = L.lib()
    lib.nm_prof_reset()
    lib.nm_prof_enable(1, None)
    try:
        out = run()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 14)
        lib.nm_prof_report(buf, len(buf))
    finally:
        lib.nm_prof_enable(0, None)
        lib.nm_prof_reset()
    return out, sorted(line.rsplit(" ", 2)[0].strip("()") for line in buf.value.decode().splitlines())


def _same_logs(la, lb):
    """two _chain logs hold the same bits, step for step"""
    assert len(la) == len(lb)
    for k, (ra, rb) in enumerate(zip(la, lb)):
        for what, x, y in zip(("state before", "rows", "state after"), ra, rb):
            assert torch.equal(x, y), (k, what, float((x - y).abs().max()), x.cpu().tolist(), y.cpu().tolist())


def _small():
    """100 particles: one scatter workgroup, whose fp64 LDS sums are exact in any order, so that two runs agree bitwise at all
    (tests/test_gpu_contact.py, the bitwise test)"""
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=100, G=16, near_wall=False)
    return const, (vol, rho, clip, en), (x, v, C_, F, S)


SPHERE = dict(type="sphere", center=[0.5, 0.42, 0.5], radius=0.1, surface="friction", friction=0.4, velocity=[0.0, 2.0, 0.5])


def _run_small(colliders, steps=8, before=None):
    const, (vol, rho, clip, en), ins = _small()
    model = _model(const, before if before is not None else colliders)
    st = build_statics(model, vol, rho, clip, en, dev())
    state = _state(model, ins)
    if before is not None:
        model.handle()
        model.set_colliders(colliders)
    outs, log = _chain(model, st, state, model.prescribed_colliders, const, steps)
    return [t.clone() for t in outs] + list(model.grid_export()), log


def test_two_runs_give_the_same_bits_and_contact_is_what_the_step_consumed():
    body = dict(SPHERE, dynamic=True, mass=5.0, angular_velocity=[3.0, 0.0, -2.0])
    (a, la), names = _kernels(lambda: _run_small([body]))
    b, lb = _run_small([body])
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    _same_logs(la, lb)
    assert float(torch.stack([r for _, r, _ in la])[:, 1, 8].min()) > 0
    assert {"k_grid_collide_rigid", "k_contact_rows_rigid", "k_contact_sum", "k_rigid_step", "k_rigid_state"} <= set(names)
    assert "k_grid_collide" not in names and "k_contact_rows" not in names
    # a body that starts at rest, without gravity: P after its first step IS the J of contact(), bit for bit, and Lc is L - c x J
    rest = dict(SPHERE, velocity=[0.0, 0.0, 0.0], dynamic=True, mass=5.0, gravity=False)
    _, log = _run_small([rest], steps=1)
    s0, rows, s1 = (t.cpu() for t in log[0])
    assert float(rows[1, 0:3].abs().max()) > 0 and torch.equal(s1[0, 7:10], rows[1, 0:3])
    want = rows[1, 3:6] - torch.linalg.cross(s0[0, 0:3], rows[1, 0:3])
    assert rc.rel(s1[0, 10:13].numpy(), want.numpy()) < 1e-13


def test_a_model_without_bodies_runs_what_it_ran():
    """set_colliders([...]) with no body: the kernels of the code as it was, by name, and - after a body was set and taken away
    again on the same handle - the same bits, step for step"""
    (a, la), names = _kernels(lambda: _run_small([SPHERE]))
    assert names == ["k_clear", "k_contact_rows", "k_contact_sum", "k_g2p", "k_grid_collide", "k_grid_export", "k_grid_op", "k_p2g"], names
    b, lb = _run_small([SPHERE], before=[dict(SPHERE, dynamic=True, mass=5.0)])
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(r[2].shape == (0, 19) for r in la + lb)
    # (the rows of two such runs are NOT compared bit for bit: k_contact_rows sums in the order of the active-block list, which the
    #  scatter's threads append to in whatever order they arrive - 1 ulp of fp64 between runs; two calls on one state agree, which is
    #  what nm_mpm_contact promises.  k_contact_rows_rigid visits the blocks by id instead: the test above holds its rows to the bit.)
    for (_, ra, _), (_, rb, _) in zip(la, lb):
        assert float((ra - rb).abs().max()) <= 1e-15 * float(ra.abs().max())
    # a prescribed mover next to a body: the host advances the one, the device the other
    const, (vol, rho, clip, en), ins = _small()
    mover = dict(type="sphere", center=[0.2, 0.8, 0.2], radius=0.05, surface="slip", velocity=[0.5, 0.0, 0.0])
    model = _model(const, [mover, dict(SPHERE, dynamic=True, mass=5.0)])
    st = build_statics(model, vol, rho, clip, en, dev())
    _, log = _chain(model, st, _state(model, ins), model.prescribed_colliders, const, 3, "rigid sphere behind a prescribed mover N=100 G=16")
    now = model.colliders
    assert abs(now[0].center[0] - (0.2 + 3 * const.dt * 0.5)) < 1e-15 and now[0].body is None
    assert now[1].center == tuple(log[2][2].cpu().numpy()[0, 0:3]) and now[1].center != (0.5, 0.42, 0.5)
    assert now[1].body.angular_velocity == tuple(log[2][2].cpu().numpy()[0, 16:19])
    assert model.prescribed_colliders[1].center == (0.5, 0.42, 0.5)


def test_refusals():
    from neuma_amd import _lib as L
    from neuma_amd import NeumaHipError
    const, (vol, rho, clip, en), ins, _ = _case(3001, 16, "noslip")
    body = rc.body_cfg("sphere", "sticky", 16)
    model = _model(const, [dict(type="plane", point=[0.5, 0.1, 0.5]), body])
    st = build_statics(model, vol, rho, clip, en, dev())
    state, nxt = _state(model, ins), model.state(3001)
    model.forward(st, state, nxt)
    with pytest.raises(NotImplementedError, match="dynamic"):
        model.backward(st, state, nxt)
    lib, h = L.lib(), model.handle()
    cst, cur = st.c_struct(), state.particle.c_struct()
    assert lib.nm_mpm_num_rigid_bodies(h) == 1
    assert lib.nm_mpm_backward(h, 3001, C.byref(cst), C.byref(cur), C.byref(cur), C.byref(cur), C.byref(cur), None) == -1
    assert b"rigid bodies: forward only" in lib.nm_last_error()
    assert lib.nm_mpm_backward_ex(h, 3001, C.byref(cst), C.byref(cur), C.byref(cur), C.byref(cur), C.byref(cur), None, 0, None) == -1
    assert b"rigid bodies: forward only" in lib.nm_last_error()
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        model.forward_extra(st, state, st, state)
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        model.shard(None)
    cfg, w = L.nm_rollout_cfg(1, 1e-3, 0, 0, 0, None, None, 0, 0), L.nm_mlp(None, None, None)
    p = L.ptr(torch.zeros(64, device=dev()))
    assert lib.nm_rollout_forward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, None, 0, None) == -1
    assert b"colliders: per-operator path only" in lib.nm_last_error()
    assert lib.nm_rollout_backward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, p, p, p, p, None, 0, None) == -1
    assert b"colliders: per-operator path only" in lib.nm_last_error()
    # the ABI's own validation, on a live handle: the message names the field, and a refused call leaves the bodies as they were
    before = model.rigid_state().clone()

    def bad(text, **kw):
        b = L.nm_rigid_body(kw.get("collider", 1), kw.get("flags", 0), kw.get("mass", 1.0), (C.c_double * 3)(*kw.get("inertia", (1.0, 1.0, 1.0))),
                            (C.c_double * 3)(*kw.get("w", (0.0, 0.0, 0.0))))
        arr = (L.nm_rigid_body * kw.get("n", 1))(*([b] * kw.get("n", 1)))
        assert lib.nm_mpm_set_rigid_bodies(h, kw.get("n", 1), arr) == -1 and text in lib.nm_last_error(), lib.nm_last_error()

    bad(b"rigid body 0: collider: entry 0 is a plane", collider=0)
    bad(b"rigid body 0: collider: index 2 outside", collider=2)                 # (a mesh entry is not in the analytic list at all)
    bad(b"rigid body 0: collider: index -1 outside", collider=-1)
    bad(b"rigid body 0: mass: must be positive", mass=0.0)
    bad(b"rigid body 0: mass: must be positive", mass=-1.0)
    bad(b"rigid body 0: mass: must be positive", mass=float("nan"))
    bad(b"rigid body 0: inertia:", inertia=(1.0, 0.0, 1.0))
    bad(b"rigid body 0: inertia:", inertia=(1.0, float("inf"), 1.0))
    bad(b"rigid body 0: angular_velocity:", w=(0.0, float("nan"), 0.0))
    bad(b"rigid body 0: flags:", flags=4)
    bad(b"rigid body 1: collider: entry 1 is a rigid body already (duplicate)", n=2)
    bad(b"rigid bodies: n = 9 outside 0..8", n=9)
    assert lib.nm_mpm_num_rigid_bodies(h) == 1 and torch.equal(model.rigid_state(), before)
    with pytest.raises(ValueError, match="collider 0: dynamic: only a sphere or a box"):
        model.set_colliders([dict(type="plane", dynamic=True, mass=1.0)])
    # a list of the same length keeps the bodies (their host pose is ignored), but a body's entry cannot become a plane
    plane = L.nm_collider(0, 0, 0.0, (C.c_float * 3)(0.5, 0.1, 0.5), (C.c_float * 3)(0.0, 1.0, 0.0), 0.0, (C.c_float * 3)(), (C.c_float * 9)(),
                          (C.c_float * 3)())
    assert lib.nm_mpm_set_colliders(h, 2, (L.nm_collider * 2)(plane, plane)) == -1 and b"collider 1: shape: the entry is a rigid body" in lib.nm_last_error()
    assert lib.nm_mpm_set_colliders(h, 1, (L.nm_collider * 1)(plane)) == 0 and lib.nm_mpm_num_rigid_bodies(h) == 0      # another length: gone
    model.set_colliders([])
    model.forward_extra(st, state, st, state)


def _read(path):
    lines = list(csv.reader(open(path)))
    return lines[0], lines[1:]


def test_inference_entry_point_with_a_falling_sphere(tmp_path, capsys):
    """`python -m neuma_amd.inference` on the one-object scene of the collider tests at G = 16 with a heavy dynamic sphere thrown
    down at the body, --draw_colliders --report_contacts: rigid_<video_name>.csv has one row per frame and body; the sphere's cy
    falls monotonically and, until its contact row holds a node, exactly as a free body; afterwards it is slower than free fall; its
    contacts row is not empty.  The same config without `dynamic` (a prescribed sphere) writes no rigid file."""
    import yaml
    from test_gpu_contact import _byte_for_byte, _files
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd.inference import main as inference_main
    from neuma_amd.rigid import CSV_COLUMNS
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"
    G, steps, v0, y0 = 16, 20, -2.0, 0.53125
    obj = dict(sim_data_name="tinyball", pretrained_ckpt=str(raw / "jelly_0300.pt"), gaussian=dict(sh_degree=3),
               particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                             sim_bounds=[[0.25, 0.02, 0.25], [0.75, 0.52, 0.75]]),
                                  vel=dict(lin_vel=[0.0, 0.0, 0.0], ang_vel=[0.0, 0.0, 0.0]), rho=1000.0, clip_bound=0.1),
               constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"], views=["r_0"]))
    sphere = dict(type="sphere", center=[0.5, y0, 0.5], radius=0.08, surface="sticky", velocity=[0.0, v0, 0.0])
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=[dict(sphere, dynamic=True, mass=50.0)]), objects=[obj])
    demo = tmp_path / "rigid-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    common = ["-s", str(steps), "-vn", "drop", "-dv", "r_0", "-sp", "drop"]
    capsys.readouterr()
    inference_main(["-c", str(demo)] + common + ["--result_root", str(tmp_path / "rigid"), "--draw_colliders", "--report_contacts"])
    out = capsys.readouterr().out
    assert "rigid body: dynamic mass=50 " in out and "colliders: 1 (drawn in renders)" in out and "rigid bodies: " in out
    head, body = _read(tmp_path / "rigid" / "inference" / "rigid_drop.csv")
    assert tuple(head) == CSV_COLUMNS and len(body) == steps and [l[0] for l in body] == [str(k) for k in range(1, steps + 1)]
    assert all(l[2] == "0:sphere" and all(math.isfinite(float(a)) for a in l[3:]) for l in body)
    chead, contacts = _read(tmp_path / "rigid" / "inference" / "contacts_drop.csv")
    mine = [l for l in contacts if l[3] == "0:sphere"]
    assert len(mine) == steps
    nodes = [float(l[12]) for l in mine]
    first = next(k for k, n in enumerate(nodes) if n > 0)          # frame index (from 0) of the first contact
    assert 2 <= first < steps - 4, nodes
    assert any(float(a) != 0.0 for a in mine[first][4:7])          # the contacts row of the body is not empty: a force on it
    dt, g = float(np.float32(cfg["sim"]["dt"])), float(np.float32(cfg["sim"]["gravity"][1]))
    cy, vy = [float(l[4]) for l in body], [float(l[11]) for l in body]
    assert all(b < a for a, b in zip([y0] + cy, cy))             # monotonically down
    for k in range(first):                                         # free flight: the closed form of the symplectic-Euler step
        n = k + 1
        assert abs(cy[k] - (y0 + n * dt * v0 + g * dt * dt * n * (n + 1) / 2)) < 1e-12
    assert all(abs(vy[k]) < abs(v0 + g * dt * (k + 1)) for k in range(first, steps))      # slower than free fall from the contact on
    imgs = sorted((tmp_path / "rigid" / "inference" / "images_drop").glob("*.png"))
    assert len(imgs) == steps + 1 and imgs[0].read_bytes() != imgs[-1].read_bytes()
    # without `dynamic`: a prescribed sphere - the files of the run above but for the two reports, no rigid file, no rigid line
    cfg["sim"]["colliders"] = [sphere]
    plain = tmp_path / "plain-tiny.yaml"
    plain.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(plain)] + common + ["--result_root", str(tmp_path / "plain"), "--draw_colliders"])
    text = capsys.readouterr().out
    assert "rigid bod" not in text and "colliders: 1 (drawn in renders)" in text
    assert not list((tmp_path / "plain").rglob("rigid_*.csv"))
    first_plain = _files(tmp_path / "plain")
    assert sorted(first_plain) == sorted(k for k in _files(tmp_path / "rigid") if not k.endswith(".csv"))

    # every byte of a body-free run against further such runs, without and with the contact report (which goes through the meter's
    # reference points and the frame writer's new branches), over the 6 frames before the moving sphere, drawn in each, reaches the
    # body.  Not further: the scatter's float atomics leave the velocities of two runs an ulp apart from the first frame on, which
    # the positions in the files do not show until a sticky contact amplifies it - measured here, 16 pairs of runs of this command
    # agreed in every byte through frame 6 and in no state file from frame 7, the contact, on (their images agreed throughout).
    # Where even these frames differ, up to three more pairs are made (tests/test_gpu_contact.py _byte_for_byte), never a tolerance.
    assert first >= 6
    short = ["-s", "6"] + common[2:]

    def again(name, extra):
        inference_main(["-c", str(plain)] + short + ["--result_root", str(tmp_path / name), "--draw_colliders"] + extra)
        assert "rigid bod" not in capsys.readouterr().out
        return _files(tmp_path / name)

    _byte_for_byte(again("plain_a", []), again("plain_flag", ["--report_contacts"]), "inference/contacts_drop.csv",
                   lambda i: again(f"plain_a{i}", []), lambda i: again(f"plain_flag{i}", ["--report_contacts"]), 6)
    runs = [again("plain_b", []), again("plain_c", [])]
    for i in range(3):
        if any(a == b for k, a in enumerate(runs) for b in runs[k + 1:]):
            break
        runs.append(again(f"plain_e{i}", []))
    assert any(a == b for k, a in enumerate(runs) for b in runs[k + 1:]) and len(runs[0]) == 2 * 6 + 1
