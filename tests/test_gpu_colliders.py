"""GPU: colliders of the per-operator MPM path (k_grid_collide / k_grid_collide_bwd behind the grid update) against the
fp64 definition neuma_amd/extras/colliders.py composed with the oracle's p2g / grid_op / g2p, plus the exact consequences,
the GridTape path, the no-collider identity, the in-place forward driver and every refusal.

Geometry: the inside test of a node is a branch, so every collider is placed with no grid node within 0.05 dx of its surface
(node coordinates are exact in fp32 for G = 16, 32; the fp32 evaluation of a signed distance is off by ~1e-7, 0.05 dx is
>= 1.5e-3), and the box additionally with no inside node whose two smallest penetration depths are within 0.02 dx of each
other (the choice of the face is a branch too).  `_check_geometry` asserts both in fp64.  For the plane n = (0.6, 0.8, 0)
the node distances are multiples of 0.2 dx, so an offset of 0.2 k + 0.1 cells keeps every node 0.1 dx away."""
import ctypes as C
import functools

import pytest
import torch

from oracle import mpm as om
from gpu_util import dev, rel_max, abs_max, mpm_case, build_model, build_statics, parity
from neuma_amd.extras import colliders as xc
from neuma_amd.sim.colliders import Box, Plane, Sphere, parse_colliders

pytestmark = pytest.mark.gpu

SIZES = [(4096, 32), (3001, 16)]
VC = (0.0531, 0.0217, -0.0293)      # a collider velocity no node normal is orthogonal or parallel to (see _check_thresholds)
MU = 0.4


def collider_cfg(shape, surface, G, velocity=VC):
    """The three test colliders as `sim.colliders` entries."""
    common = dict(surface=surface, friction=MU if surface == "friction" else 0.0, velocity=list(velocity))
    if shape == "plane":      # through the middle of the cloud: (0.5, 0.5, 0.5).n = 0.7 = 22.4 cells (G = 32) / 11.2 (G = 16)
        off = {32: 22.5, 16: 11.3}[G] / G
        return dict(type="plane", point=[0.6 * off, 0.8 * off, 0.0], normal=[0.6, 0.8, 0.0], **common)
    if shape == "sphere":
        return dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.12, **common)
    # box turned about z onto the axes a = (0.6, 0.8, 0), b = (-0.8, 0.6, 0), c = z.  In cells: node coordinates along a and b are
    # multiples of 0.2, along c integers.  The centre sits at a multiple of 0.2 along a, 0.03 off one along b, at an integer
    # along c, and the half extents are 0.1, 0.1 and 0.0 (mod 0.2): penetration depths are then 0.1 (a), 0.07 / 0.13 (b) and 0.0
    # (c) mod 0.2 - no node within 0.07 cells of a face, no two depths of a node within 0.03 cells of each other.
    ctr, half = {32: ((16, 15, 16), (4.7, 2.5, 3.6)), 16: ((8, 7, 8), (2.3, 1.3, 1.6))}[G]
    center = [(ctr[0] - 0.03 * 0.8) / G, (ctr[1] + 0.03 * 0.6) / G, ctr[2] / G]
    return dict(type="box", center=center, half=[h / G for h in half], rot=[[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]],
                **common)


def _check_geometry(colliders, G):
    """fp64: no node within 0.05 dx of a surface; no inside node of a box within 0.02 dx of a change of face."""
    p = xc.node_positions(G)
    for c in colliders:
        if isinstance(c, Box):
            q, pen = xc.box_penetration(c, p)
            e = -pen
            dist = torch.where((e < 0).all(-1), e.max(-1).values, e.clamp_min(0.0).norm(dim=-1))
            srt = pen[(pen > 0).all(-1)].sort(dim=-1).values
            assert srt.shape[0] > 0 and float((srt[:, 1] - srt[:, 0]).min()) * G > 0.02, "box: a node next to a change of face"
        else:
            dist = xc.sdf_normal(c, p)[0]
        assert int((dist < 0).sum()) > 0, "collider holds no node"
        assert float(dist.abs().min()) * G > 0.05, f"{type(c).__name__}: a node within 0.05 dx of the surface"


@functools.lru_cache(maxsize=None)
def _case(N, G, bc, seed=0):
    """mpm_case rounded to fp32 (what the GPU sees) and the oracle's grid behind the box boundary condition: computed once per
    (size, bc, seed) and shared by every collider case; nothing modifies it."""
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=N, G=G, bc=bc, seed=seed)
    ins = tuple(t.float().double() for t in (x, v, C_, F, S))
    gmv, gm = om.p2g(const, vol, rho, en, ins[0], ins[1], ins[2], ins[4])
    gv = om.grid_op(const, gmv, gm)
    return const, (vol, rho, clip, en), ins, (gmv, gm, gv)


def _model(const, colliders):
    model = build_model(const, dev())
    model.set_colliders(colliders)
    return model


def _gpu_step(model, st, ins):
    from neuma_amd.sim import MPMDiffSim
    gin = [t.float().to(dev()).requires_grad_(True) for t in ins]
    return gin, MPMDiffSim(model, reorder=False)(st, *gin)


@pytest.mark.parametrize("bc", ["noslip", "freeslip"])
@pytest.mark.parametrize("N,G", SIZES)
@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
@pytest.mark.parametrize("shape", ["plane", "sphere", "box"])
def test_forward_one_step_with_a_collider(shape, surface, N, G, bc):
    """One substep vs p2g -> grid_op -> collider (fp64 definition) -> g2p on the fp32 inputs.  The response is continuous across
    its velocity thresholds, so every node and every enabled particle is compared.  Bounds: those of test_forward_one_step."""
    const, (vol, rho, clip, en), ins, (gmv, gm, gv) = _case(N, G, bc)
    cs = parse_colliders([collider_cfg(shape, surface, G)])
    _check_geometry(cs, G)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    _, outs = _gpu_step(model, st, ins)
    gvc = xc.apply_colliders(cs, gv, G)
    assert int(((gvc != gv).any(-1) & (gm > 0)).sum()) >= 8, "the collider changes (almost) no node that holds mass"
    ox, ov, oC, oF = om.g2p(const, clip, en, ins[0], ins[3], gvc, ins[1], ins[2])
    mv, m, vg = model.grid_export()
    case = f"collider {shape}/{surface} N={N} G={G} {bc} vs fp64 definition"
    parity(case, "grid v (mass-weighted)", rel_max(vg * m[..., None], gvc * gm[..., None]), 7e-7)      # measured <= 1.8e-7 over the 36 cases
    e = (en != 0)
    parity(case, "x", abs_max(outs[0][e], ox[e]), 1e-7)            # 3.0e-8
    parity(case, "v", rel_max(outs[1][e], ov[e]), 7e-7)            # 2.4e-7
    parity(case, "C", rel_max(outs[2][e], oC[e]), 1e-6)            # 2.8e-7
    parity(case, "F", abs_max(outs[3][e], oF[e]), 7e-7)            # 2.3e-7
    # nodes in blocks no particle touches: the dense definition collides them too (grid_export only; nothing gathers from them)
    empty = (gm == 0)
    assert abs_max(vg.cpu()[empty], gvc[empty]) < 1e-7      # measured 3.2e-9 (|u| there is |g dt - v_c| ~ 0.07: fp32 rounding)


ADJ_SEED = 0      # mpm_case seed of the adjoint cases: chosen on the CPU so that _check_thresholds holds for all six


def _check_thresholds(cs, gv, G):
    """fp64: no node inside a collider sits at a jump of the Jacobian: |vn| >= 1e-4 |w|, |vt| >= 1e-4 |w|, and for friction
    |1 + mu vn / |vt|| >= 1e-4 where the node approaches.  (Every node of the dense grid, with or without mass.)"""
    p = xc.node_positions(G)
    u = gv.reshape(-1, 3)
    for c in cs:
        sdf, n = xc.sdf_normal(c, p)
        ins = sdf < 0
        w = (u - torch.tensor(c.velocity, dtype=u.dtype))[ins]
        vn = (w * n[ins]).sum(-1)
        vt = w - vn[:, None] * n[ins]
        s, wl = vt.norm(dim=-1), w.norm(dim=-1)
        assert not bool((vn.abs() < 1e-4 * wl).any()), "a colliding node with |vn| < 1e-4 |w|"
        assert not bool((s < 1e-4 * wl).any()), "a colliding node with |vt| < 1e-4 |w|"
        if c.surface == "friction":
            app = vn < 0
            assert not bool(((1.0 + c.friction * vn[app] / s[app]).abs() < 1e-4).any()), "a colliding node at the edge of the Coulomb cone"
        u = xc.apply_collider(c, p, u)


@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
@pytest.mark.parametrize("shape,bc", [("plane", "noslip"), ("sphere", "freeslip")])
def test_backward_one_step_with_a_collider(shape, bc, surface):
    """One substep's adjoint vs fp64 autograd of p2g -> grid_op -> collider -> g2p.  The Jacobian of the response jumps at vn = 0,
    |vt| = 0 and at the edge of the Coulomb cone: the case (seed ADJ_SEED) has no colliding node near any of them, asserted."""
    N, G = 4096, 32
    const, (vol, rho, clip, en), ins, (_, _, gv) = _case(N, G, bc, ADJ_SEED)
    cs = parse_colliders([collider_cfg(shape, surface, G)])
    _check_geometry(cs, G)
    _check_thresholds(cs, gv, G)
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    gin, outs = _gpu_step(model, st, ins)
    torch.manual_seed(11)
    gws = [torch.randn(o.shape) for o in outs]
    grads = torch.autograd.grad(sum((o * g.to(dev())).sum() for o, g in zip(outs, gws)), gin)
    oins = [t.clone().requires_grad_(True) for t in ins]
    gmv, gm = om.p2g(const, vol, rho, en, oins[0], oins[1], oins[2], oins[4])
    gvc = xc.apply_colliders(cs, om.grid_op(const, gmv, gm), G)
    oo = om.g2p(const, clip, en, oins[0], oins[3], gvc, oins[1], oins[2])
    og = torch.autograd.grad(sum((o * g.double()).sum() for o, g in zip(oo, gws)), oins)
    for nme, a, b in zip(["x", "v", "C", "F", "stress"], grads, og):
        parity(f"collider {shape}/{surface} one-step adjoint N={N} G={G} {bc} vs fp64 autograd", f"dL/d{nme} (rel)", rel_max(a, b), 8e-6)      # measured: dL/dx 2.5e-6, the others <= 3.5e-7
        assert torch.isfinite(a).all()


def _planted_case(G=32):
    """_case(4096, 32) with its first 8 enabled particles moved next to the centre, so that their whole 27-node stencils lie
    inside the 0.12 sphere (asserted)."""
    const, (vol, rho, clip, en), ins, _ = _case(4096, G, "noslip")
    idx = torch.nonzero(en != 0)[:8, 0]
    x = ins[0].clone()
    x[idx] = (0.5 + 0.4 / G * (torch.rand(8, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5)).float().double()
    base, _, _ = om._stencil(const, x[idx])
    off, _ = om._offsets(torch.float64)
    nodes = (base[:, None, :] + off[None]).double() / G
    assert float((nodes - 0.5).norm(dim=-1).max()) < 0.12 - 0.05 / G
    return const, (vol, rho, clip, en), (x,) + tuple(ins[1:]), idx


@pytest.mark.parametrize("vc", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.1)])
def test_particle_inside_a_sticky_collider_takes_its_velocity(vc):
    """Every node of the stencil holds v_c, and the 27 fp32 weights sum to 1 within about 27 ulp: the next velocity is v_c within
    4e-6 relative - and exactly 0 for a static collider."""
    const, (vol, rho, clip, en), ins, idx = _planted_case()
    model = _model(const, [dict(type="sphere", center=[0.5, 0.5, 0.5], radius=0.12, surface="sticky", velocity=list(vc))])
    st = build_statics(model, vol, rho, clip, en, dev())
    _, outs = _gpu_step(model, st, ins)
    vn = outs[1].detach().cpu().double()[idx]
    if not any(vc):
        assert torch.equal(vn, torch.zeros_like(vn))
    else:
        assert rel_max(vn, torch.tensor(vc, dtype=torch.float64).expand_as(vn)) < 4e-6      # measured 1.4e-7


@pytest.mark.parametrize("N,G", SIZES)
def test_no_node_inside_a_slip_half_space_approaches_it(N, G):
    const, (vol, rho, clip, en), ins, _ = _case(N, G, "freeslip")
    cs = parse_colliders([collider_cfg("plane", "slip", G, velocity=(0.0, 0.0, 0.0))])
    model = _model(const, cs)
    st = build_statics(model, vol, rho, clip, en, dev())
    _gpu_step(model, st, ins)
    _, _, vg = model.grid_export()
    u = vg.cpu().double().reshape(-1, 3)
    sdf, n = xc.sdf_normal(cs[0], xc.node_positions(G))
    assert float((u[sdf < 0] @ n[0]).min()) >= -1e-6 * float(u.abs().max())      # four times the fp32 rounding of the projection


def test_grid_tape_with_a_collider_matches_recompute():
    """As test_per_operator_grid_tape_matches_recompute, with a collider set: the backward pass through a restored record (and
    through an overflowed one) gives the gradients of the recompute path."""
    from neuma_amd.sim import MPMCacheDiffSim
    const, (vol, rho, clip, en), ins, _ = _case(4096, 32, "noslip")
    res = {}
    for tag, cache in (("recompute", 0), ("auto", "auto"), ("overflow", 1)):
        model = _model(const, [collider_cfg("plane", "friction", 32), collider_cfg("sphere", "slip", 32)])
        model.grid_cache = cache
        st = build_statics(model, vol, rho, clip, en, dev())
        sim = MPMCacheDiffSim(model, 3, reorder=False)
        gin = [t.float().to(dev()).requires_grad_(True) for t in ins]
        a = sim(st, 0, *gin)
        b = sim(st, 1, a[0], a[1], a[2], a[3], gin[4])          # second substep: the auto capacity is known by now
        if cache == "auto":
            assert model._cache_blocks is not None and model.new_tape() is not None
        res[tag] = torch.autograd.grad(b[0].sum() + (b[3] * b[3]).sum() + b[1].sum(), gin)
    for tag in ("auto", "overflow"):
        for g, r in zip(res[tag], res["recompute"]):
            assert rel_max(g, r) < 1.5e-6, tag      # measured 3.3e-07


def test_an_empty_collider_list_is_bitwise_the_model_without_colliders():
    """set_colliders([]) after colliders, `colliders: []` and a config without the key: the same launches as ever, bitwise the same
    outputs and gradients.  (100 particles: one scatter workgroup, whose fp64 LDS sums of fp32 terms are exact in any order - with
    several workgroups the order of their global float atomics is free, and two runs of ONE model may differ in the last bit.)"""
    from neuma_amd.sim import MPMModelBuilder
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=100, G=16, near_wall=False)
    ins = (x, v, C_, F, S)
    cfg = dict(gravity=list(const.gravity), bc=const.bc, num_grids=const.num_grids, dt=const.dt, bound=const.bound, eps=const.eps)
    torch.manual_seed(5)
    gws = None
    res = []
    for kind in ("fresh", "emptied", "empty key"):
        model = MPMModelBuilder().parse_cfg(dict(cfg, colliders=[]) if kind == "empty key" else cfg).finalize(dev(), requires_grad=True)
        st = build_statics(model, vol, rho, clip, en, dev())
        if kind == "emptied":
            model.set_colliders([collider_cfg("sphere", "sticky", 16)])
            _, changed = _gpu_step(model, st, ins)
            model.set_colliders([])
        assert model.colliders == []
        gin, outs = _gpu_step(model, st, ins)
        gws = gws or [torch.randn(o.shape, device=dev()) for o in outs]
        grads = torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gws)), gin)
        res.append([t.detach().clone() for t in outs] + list(grads) + list(model.grid_export()))
        if kind == "emptied":
            assert not torch.equal(changed[1], outs[1])          # (the collider did act before it was removed)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


def test_forward_sim_steps_in_place_against_moving_colliders():
    from neuma_amd.sim import MPMForwardSim, MPMModelBuilder
    const, (vol, rho, clip, en), ins, _ = _case(3001, 16, "freeslip")
    vel = [0.0, 0.5, 0.25]
    cfg = dict(gravity=list(const.gravity), bc=const.bc, num_grids=const.num_grids, dt=const.dt, bound=const.bound, eps=const.eps,
               colliders=[dict(type="plane", point=[0.5, 0.32, 0.5], normal=[0.2, 1, 0], surface="friction", friction=0.4),
                          dict(type="sphere", center=[0.5, 0.4, 0.5], radius=0.08, surface="slip", velocity=vel),
                          dict(type="box", center=[0.4, 0.5, 0.6], half=[0.1, 0.05, 0.1], euler_xyz_deg=[0, 0, 20], surface="sticky")])
    model = MPMModelBuilder().parse_cfg(cfg).finalize(dev())
    assert [type(c) for c in model.colliders] == [Plane, Sphere, Box]
    st = build_statics(model, vol, rho, clip, en, dev())
    state = model.state(3001)
    state.from_torch(**{k: t.float().to(dev()) for k, t in zip(("x", "v", "C", "F", "stress"), ins)})
    held = state.to_torch()[0]
    sim = MPMForwardSim(model)
    for _ in range(20):
        outs = sim(st, state)
        model.step_colliders()
    assert outs[0].data_ptr() == held.data_ptr()
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    moved = model.colliders[1].center
    for a, c0, vv in zip(moved, (0.5, 0.4, 0.5), vel):
        assert abs(a - (c0 + 20 * const.dt * vv)) < 1e-15
    assert model.colliders[0].point == (0.5, 0.32, 0.5) and model.colliders[2].center == (0.4, 0.5, 0.6)
    static = MPMModelBuilder().parse_cfg(dict(cfg, colliders=cfg["colliders"][:1])).finalize(dev())
    static.step_colliders()                                      # nothing moves: nothing happens
    assert static.colliders[0].point == (0.5, 0.32, 0.5)


def test_every_other_path_refuses_colliders():
    from neuma_amd import _lib as L
    from neuma_amd import NeumaHipError
    const, (vol, rho, clip, en), ins, _ = _case(3001, 16, "noslip")
    model = _model(const, [collider_cfg("sphere", "sticky", 16)])
    st = build_statics(model, vol, rho, clip, en, dev())
    state = model.state(3001)
    state.from_torch(**{k: t.float().to(dev()) for k, t in zip(("x", "v", "C", "F", "stress"), ins)})
    lib, h = L.lib(), model.handle()
    msg = b"colliders: per-operator path only"
    cfg = L.nm_rollout_cfg(1, 1e-3, 0, 0, 0, None, None, 0, 0)
    cst, cur, w = st.c_struct(), state.particle.c_struct(), L.nm_mlp(None, None, None)
    buf = torch.zeros(64, device=dev())
    p = L.ptr(buf)
    assert lib.nm_rollout_forward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, None, 0, None) == -1
    assert msg in lib.nm_last_error()
    assert lib.nm_rollout_backward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, p, p, p, p, None, 0, None) == -1
    assert msg in lib.nm_last_error()
    assert lib.nm_rollout_forward_sharded(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, None, 0, None, 1, 1,
                                          None, 0, None) == -1
    assert msg in lib.nm_last_error()
    assert lib.nm_rollout_backward_sharded(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, p, p, p, p, None, 0,
                                           None, 1, 1, None, 0, None) == -1
    assert msg in lib.nm_last_error()
    for call in (lambda: lib.nm_mpm_p2g(h, 3001, C.byref(cst), C.byref(cur), None),
                 lambda: lib.nm_mpm_forward_finish(h, 3001, C.byref(cst), C.byref(cur), C.byref(cur), None, 0, None, None),
                 lambda: lib.nm_mpm_backward_begin(h, 3001, C.byref(cst), C.byref(cur), C.byref(cur), C.byref(cur), C.byref(cur), p, 1, None),
                 lambda: lib.nm_mpm_backward_finish(h, 3001, C.byref(cst), C.byref(cur), C.byref(cur), None)):
        assert call() == -1
        assert msg in lib.nm_last_error()
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        model.forward_extra(st, state, st, state)
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):
        model.shard(None)
    # the ABI's own validation, on a live handle: the message names the field, and a refused call leaves the set as it was
    bad = L.nm_collider(1, 0, 0.0, (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(), -1.0, (C.c_float * 3)(), (C.c_float * 9)(),
                        (C.c_float * 3)())
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"radius" in lib.nm_last_error()
    bad.shape, bad.normal = 0, (C.c_float * 3)(0.0, 0.9, 0.0)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"normal" in lib.nm_last_error()
    bad.shape = 7
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"shape" in lib.nm_last_error()
    bad.shape, bad.surface = 1, 5
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"surface" in lib.nm_last_error()
    bad.surface, bad.radius, bad.friction = 2, 0.1, -0.5
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"friction" in lib.nm_last_error()
    bad.shape, bad.friction, bad.half = 2, 0.0, (C.c_float * 3)(0.1, 0.1, 0.0)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"half" in lib.nm_last_error()
    bad.half = (C.c_float * 3)(0.1, 0.1, 0.1)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"rot" in lib.nm_last_error()      # all-zero rotation
    bad.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, -1)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"rot: not orthonormal (a reflection" in lib.nm_last_error()
    bad.rot, bad.center = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0.5, float("nan"), 0.5)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"center" in lib.nm_last_error()
    bad.center, bad.velocity = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.0, float("inf"), 0.0)
    assert lib.nm_mpm_set_colliders(h, 1, C.byref(bad)) == -1 and b"velocity" in lib.nm_last_error()
    assert lib.nm_mpm_set_colliders(h, 9, C.byref(bad)) == -1 and b"outside 0..8" in lib.nm_last_error()
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):                       # still set
        model.forward_extra(st, state, st, state)
    model.set_colliders([])
    model.forward_extra(st, state, st, state)                      # and accepted again once they are gone


def test_simulate_objects_steps_against_colliders_and_moves_them():
    """The multi-object forward driver behind `python -m neuma_amd.inference` (infer.simulate_objects; the scene helper is the one
    of tests/test_gpu_infer.py) with a sticky half-space through the first body and a moving sphere: particles deep inside the
    half-space stand still from the first frame on, the rest of the body falls, and the driver advances the sphere once per step."""
    from test_gpu_infer import _object
    from neuma_amd import synth
    from neuma_amd.infer import simulate_objects
    from neuma_amd.sim import MPMModelBuilder
    G, steps, d = 32, 4, dev()
    vel = (0.0, 0.25, 0.0)
    model = MPMModelBuilder().parse_cfg(dict(
        gravity=[0.0, -9.8, 0.0], bc="noslip", num_grids=G, dt=1e-3, bound=1, eps=6e-7,
        colliders=[dict(type="plane", point=[0.3, 0.5 + 1.1 / G, 0.3], normal=[0, 1, 0], surface="sticky"),
                   dict(type="sphere", center=[0.7, 0.2, 0.7], radius=0.05, surface="slip", velocity=list(vel))])).finalize(d)
    o1, _, _ = _object((0.3, 0.5, 0.3), 700, G, "jelly", (0, 10 ** 9), d, seed=0)
    o2, _, _ = _object((0.7, 0.5, 0.7), 500, G, "sand", (0, 10 ** 9), d, seed=1)
    n1 = o1.init_data.num_particles
    frames = list(simulate_objects(model, [o1, o2], steps, synth.ring_cameras(1, 48, 32, device=d), torch.ones(3, device=d),
                                   denormalize=True))
    assert len(frames) == steps + 1 and all(bool(torch.isfinite(f["x"]).all()) and len(f["images"]) == 1 for f in frames)
    x0 = torch.tensor(o1.init_data.pos)
    deep = x0[:, 1] < 0.5 - 0.5 / G              # highest stencil node <= y G + 1.5 < 17.1 cells: the whole stencil is inside
    above = x0[:, 1] > 0.5 + 2.0 / G             # part of the stencil is above the surface
    assert int(deep.sum()) > 20 and int(above.sum()) > 20
    x1, xs = frames[1]["x"].cpu()[:n1], frames[steps]["x"].cpu()[:n1]
    assert torch.equal(xs[deep], x1[deep]) and abs_max(x1[deep], x0[deep]) < 1e-7      # v = 0 exactly: x + dt 0 (x0 is rounded to fp32 once)
    assert float((x1[above, 1] - xs[above, 1]).min()) > 1e-5                              # the free part keeps falling (0.5 per unit time)
    assert abs_max(frames[steps]["x"][n1:, 1], torch.tensor(o2.init_data.pos)[:, 1]) > 1e-4
    moved = model.colliders[1].center
    assert all(abs(a - (c0 + steps * 1e-3 * v)) < 1e-15 for a, c0, v in zip(moved, (0.7, 0.2, 0.7), vel))
    assert model.colliders[0].point == (0.3, 0.5 + 1.1 / G, 0.3)


def test_inference_entry_point_with_a_plane_collider(tmp_path, capsys):
    """`python -m neuma_amd.inference` on a two-object scene (the experiment writer of tests/test_gpu_entrypoints.py and the demo
    schema of its test_inference_entry_point_two_objects: one body above the other) whose YAML carries `sim.colliders`: a sticky
    half-space between the bodies and a moving sphere away from both.  The parsed colliders are printed at start-up; in the saved
    states the lower body, wholly inside the half-space, never moves, while the upper one falls; a config without the key prints
    no collider line."""
    import shutil
    import numpy as np
    import yaml
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import io as nio, synth
    from neuma_amd.config import load_config
    from neuma_amd.inference import load_object, main as inference_main
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))},
               raw / "plasticine_0300.pt")
    shutil.copytree(assets / "tinyball", assets / "tinycat")
    for f in (assets / "tinycat").glob("particles.npz"):
        f.unlink()

    def obj(name, ckpt, lo):
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=dict(sh_degree=3),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 0.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"],
                                      views=["r_0"]))

    G, steps = 32, 8
    # the bodies span y = 0.21 .. 0.33 and 0.64 .. 0.76: the plane at 14.6 cells (0.456) holds every stencil node of the lower one
    # (<= 12 cells) and none of the upper one (>= 18 cells)
    colliders = [dict(type="plane", point=[0.5, 14.6 / G, 0.5], normal=[0, 2, 0], surface="sticky"),
                 dict(type="sphere", center=[0.1, 0.9, 0.1], radius=0.04, surface="slip", velocity=[0.5, 0, 0])]
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=colliders),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "colliders-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    capsys.readouterr()
    inference_main(["-c", str(demo), "-s", str(steps), "-vn", "col", "-dv", "r_0", "-sp", "col", "--result_root", str(tmp_path / "results")])
    out = capsys.readouterr().out
    assert "colliders: 2 (not drawn in renders)" in out
    assert "[0] plane point=(0.5, 0.45625, 0.5) normal=(0.0, 1.0, 0.0) surface=sticky" in out      # normal normalised
    assert "[1] sphere center=(0.1, 0.9, 0.1) radius=0.04 surface=slip velocity=(0.5, 0.0, 0.0)" in out
    st_root = tmp_path / "results" / "inference_states" / "states_col"
    xs = [nio.load_particles_ply(st_root / f"{i:03d}.ply") for i in range(1, steps + 1)]
    objects = [load_object(o, assets, steps, dev()) for o in load_config(demo).objects]
    n0, n1 = (o.init_data.num_particles for o in objects)
    assert xs[0].shape == (n0 + n1, 3) and all(np.isfinite(x).all() for x in xs)
    lower0 = np.asarray(objects[1].init_data.pos)
    assert lower0[:, 1].max() * G + 1.5 < 14.6 and np.asarray(objects[0].init_data.pos)[:, 1].min() * G - 1.5 > 14.6
    assert all(np.array_equal(x[n0:], xs[0][n0:]) for x in xs[1:])                     # sticky, static: v = 0 exactly
    assert np.abs(xs[0][n0:] - lower0).max() < 1e-7                                     # (the start positions, rounded to fp32 once)
    upper0 = np.asarray(objects[0].init_data.pos)
    assert xs[-1][:n0, 1].mean() < upper0[:, 1].mean() - 0.8 * steps * 1e-3 * 0.5       # the upper body falls freely (0.5 per unit time)
    # a config without the key: no collider line, and the lower body falls too
    del cfg["sim"]["colliders"]
    plain = tmp_path / "plain-tiny.yaml"
    plain.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(plain), "-s", "2", "-vn", "plain", "-dv", "r_0", "-sp", "plain", "--result_root", str(tmp_path / "results")])
    assert "colliders" not in capsys.readouterr().out
    x2 = nio.load_particles_ply(tmp_path / "results" / "inference_states" / "states_plain" / "002.ply")
    assert x2[n0:, 1].mean() < lower0[:, 1].mean() - 5e-4
