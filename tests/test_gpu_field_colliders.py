"""GPU: mesh / field colliders of the per-operator MPM path (k_grid_collide_field / k_grid_collide_field_bwd behind the analytic
colliders) against the fp64 definition neuma_amd/extras/colliders.py apply_field_collider composed with the oracle's p2g /
grid_op / g2p, as tests/test_gpu_colliders.py composes the analytic ones; plus the exact consequences, the GridTape path, the
empty-list identity, the in-place forward driver, every refusal and the inference entry point.

Cases (tests/field_collider_cases.py, chosen and asserted on the CPU): torus and rotated box, each on a dyadic lattice (q exact in
fp32) and on an odd one; in the fp64 reference no node with mass has |phi| < 1e-5, a fraction within 1e-5 of a cell face (odd
lattice) or sits at a jump of the response's Jacobian.  Bounds: the collider-free substep's (x 1e-7, v 7e-7, C 1e-6, F 7e-7, node
velocity 7e-7, adjoint 8e-6 relative).  The normal is a difference of phi values: where the definition evaluated in fp32 (the
collider alone; everything around it stays fp64) is itself farther than a quarter of a bound from fp64, the bound of that
quantity in that case is 4 x that distance, and the log says so.  Measured values: profiles/mesh_sdf_parity_table.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_collider_cases as fcc
import mesh_sdf_cases as cases
from oracle import mpm as om
from gpu_util import dev, rel_max, abs_max, build_model, build_statics, parity
from neuma_amd.extras import colliders as xc
from neuma_amd.sim.colliders import MeshCollider, Sphere

pytestmark = pytest.mark.gpu


def _model(const, colliders):
    model = build_model(const, dev())
    model.set_colliders(colliders)
    return model


def _gpu_step(model, st, ins):
    from neuma_amd.sim import MPMDiffSim
    gin = [t.float().to(dev()).requires_grad_(True) for t in ins]
    return gin, MPMDiffSim(model, reorder=False)(st, *gin)


def _fp32_collider(c, u, G):
    """the definition with the collider evaluated in fp32 (positions, phi, velocities), differentiable, back in fp64"""
    return xc.apply_colliders([c], u.float(), G).double()


def _bound(case, name, measured, base, restated):
    """parity() against `base`, or against 4 x the fp32 restatement's own distance where that exceeds a quarter of `base`"""
    wide = float(restated) > base / 4
    parity(case + (" [bound: 4 x fp32 restatement]" if wide else ""), name, measured, 4.0 * float(restated) if wide else base,
           noise=float(restated))


@pytest.mark.parametrize("bc", ["noslip", "freeslip"])
@pytest.mark.parametrize("N,G", fcc.SIZES)
@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
@pytest.mark.parametrize("kind", ["dyadic", "odd"])
@pytest.mark.parametrize("mesh", ["torus", "box"])
def test_forward_one_step_with_a_field_collider(mesh, kind, surface, N, G, bc):
    const, (vol, rho, clip, en), ins, (gmv, gm, gv) = fcc.mpm_grid(N, G, bc)
    c = fcc.collider(mesh, kind, surface)
    fcc.assert_clean([c], gv, gm, G, kind)
    model = _model(const, [c])
    assert model.colliders == [] and len(model.field_colliders) == 1 and model.field_colliders[0].phi.is_cuda
    st = build_statics(model, vol, rho, clip, en, dev())
    _, outs = _gpu_step(model, st, ins)
    gvc = xc.apply_colliders([c], gv, G)
    assert int(((gvc != gv).any(-1) & (gm > 0)).sum()) >= 8, "the collider changes (almost) no node that holds mass"
    gv32 = _fp32_collider(c, gv, G)
    ref = om.g2p(const, clip, en, ins[0], ins[3], gvc, ins[1], ins[2])
    r32 = om.g2p(const, clip, en, ins[0], ins[3], gv32, ins[1], ins[2])
    mv, m, vg = model.grid_export()
    case = f"field collider {mesh}/{kind}/{surface} N={N} G={G} {bc} vs fp64 definition"
    e = (en != 0)
    _bound(case, "grid v (mass-weighted)", rel_max(vg * m[..., None], gvc * gm[..., None]), fcc.BOUNDS["grid v (mass-weighted)"],
           rel_max(gv32 * gm[..., None], gvc * gm[..., None]))
    _bound(case, "x", abs_max(outs[0][e], ref[0][e]), fcc.BOUNDS["x"], abs_max(r32[0][e], ref[0][e]))
    _bound(case, "v", rel_max(outs[1][e], ref[1][e]), fcc.BOUNDS["v"], rel_max(r32[1][e], ref[1][e]))
    _bound(case, "C", rel_max(outs[2][e], ref[2][e]), fcc.BOUNDS["C"], rel_max(r32[2][e], ref[2][e]))
    _bound(case, "F", abs_max(outs[3][e], ref[3][e]), fcc.BOUNDS["F"], abs_max(r32[3][e], ref[3][e]))
    # nodes in blocks no particle touches: the dense definition collides them too (grid_export only; nothing gathers from them).
    # Without mass behind them these nodes were not part of the choice of the case: those at a branch are left out, under the cap.
    shaky = fcc.unsafe_nodes([c], gv, gm, G, kind, with_mass=False).reshape(G, G, G)
    empty = (gm == 0)
    assert int((shaky & empty).sum()) <= fcc.EXCLUDE_CAP * int(empty.sum())
    keep = empty & ~shaky
    _bound(case, "v of empty nodes (abs)", abs_max(vg.cpu()[keep], gvc[keep]), 1e-7, abs_max(gv32[keep], gvc[keep]))


@pytest.mark.parametrize("surface", ["sticky", "slip", "friction"])
@pytest.mark.parametrize("mesh,kind,bc", [("torus", "dyadic", "noslip"), ("box", "odd", "freeslip")])
def test_backward_one_step_with_a_field_collider(mesh, kind, bc, surface):
    """One substep's adjoint vs fp64 autograd of p2g -> grid_op -> field collider -> g2p (the case is clean: asserted)."""
    N, G = 4096, 32
    const, (vol, rho, clip, en), ins, (_, gm0, gv0) = fcc.mpm_grid(N, G, bc)
    c = fcc.collider(mesh, kind, surface)
    fcc.assert_clean([c], gv0, gm0, G, kind)
    model = _model(const, [c])
    st = build_statics(model, vol, rho, clip, en, dev())
    gin, outs = _gpu_step(model, st, ins)
    torch.manual_seed(11)
    gws = [torch.randn(o.shape) for o in outs]
    grads = torch.autograd.grad(sum((o * g.to(dev())).sum() for o, g in zip(outs, gws)), gin)

    def reference(collide):
        oins = [t.clone().requires_grad_(True) for t in ins]
        gmv, gm = om.p2g(const, vol, rho, en, oins[0], oins[1], oins[2], oins[4])
        oo = om.g2p(const, clip, en, oins[0], oins[3], collide(om.grid_op(const, gmv, gm)), oins[1], oins[2])
        return torch.autograd.grad(sum((o * g.double()).sum() for o, g in zip(oo, gws)), oins)

    og = reference(lambda u: xc.apply_colliders([c], u, G))
    o32 = reference(lambda u: _fp32_collider(c, u, G))
    case = f"field collider {mesh}/{kind}/{surface} one-step adjoint N={N} G={G} {bc} vs fp64 autograd"
    for nme, a, b, r in zip(["x", "v", "C", "F", "stress"], grads, og, o32):
        _bound(case, f"dL/d{nme} (rel)", rel_max(a, b), fcc.ADJ_BOUND, rel_max(r, b))
        assert torch.isfinite(a).all()


def test_field_colliders_act_behind_the_analytic_ones_in_list_order():
    """a sphere, then the torus and the box fields: forward and adjoint against the composition in that order"""
    N, G, bc = 4096, 32, "noslip"
    const, (vol, rho, clip, en), ins, (_, gm0, gv0) = fcc.mpm_grid(N, G, bc)
    sph = Sphere(center=(0.5, 0.5, 0.5), radius=0.12, surface="slip", velocity=fcc.VC)
    cs = [sph, fcc.collider("torus", "dyadic", "friction"), fcc.collider("box", "odd", "slip", velocity=(0.0, 0.1, 0.0))]
    fcc.assert_clean(cs[1:], xc.apply_colliders([sph], gv0, G), gm0, G, ["dyadic", "odd"])
    model = _model(const, cs)
    assert len(model.colliders) == 1 and len(model.field_colliders) == 2
    st = build_statics(model, vol, rho, clip, en, dev())
    gin, outs = _gpu_step(model, st, ins)
    torch.manual_seed(11)
    gws = [torch.randn(o.shape) for o in outs]
    grads = torch.autograd.grad(sum((o * g.to(dev())).sum() for o, g in zip(outs, gws)), gin)
    oins = [t.clone().requires_grad_(True) for t in ins]
    gmv, gm = om.p2g(const, vol, rho, en, oins[0], oins[1], oins[2], oins[4])
    oo = om.g2p(const, clip, en, oins[0], oins[3], xc.apply_colliders(cs, om.grid_op(const, gmv, gm), G), oins[1], oins[2])
    og = torch.autograd.grad(sum((o * g.double()).sum() for o, g in zip(oo, gws)), oins)
    e = (en != 0)
    case = "sphere + two field colliders N=4096 G=32 noslip vs fp64 definition"
    parity(case, "v", rel_max(outs[1][e], oo[1][e]), fcc.BOUNDS["v"])
    parity(case, "C", rel_max(outs[2][e], oo[2][e]), fcc.BOUNDS["C"])
    for nme, a, b in zip(["x", "v", "C", "F", "stress"], grads, og):
        parity(case, f"dL/d{nme} (rel)", rel_max(a, b), fcc.ADJ_BOUND)
    # the other order of the two fields is another function
    swapped = xc.apply_colliders([cs[0], cs[2], cs[1]], gv0, G)
    assert float((swapped - xc.apply_colliders(cs, gv0, G)).abs().max()) > 1e-3


def _cube_mesh(lo, hi):
    v = np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)
    t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], dtype=np.int64)
    return v, cases._outward(v, t)


@pytest.mark.parametrize("vc", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.1)])
def test_particle_inside_a_sticky_mesh_collider_takes_its_velocity(vc):
    """8 particles next to the centre of a cube mesh, their whole 27-node stencils inside it (asserted on the field the model
    built): every node of the stencil holds v_c - exactly 0 for a static collider, v_c within 4e-6 relative otherwise (the 27 fp32
    weights sum to 1 within about 27 ulp)."""
    G = 32
    const, (vol, rho, clip, en), ins, _ = fcc.mpm_grid(4096, G, "noslip")
    idx = torch.nonzero(en != 0)[:8, 0]
    x = ins[0].clone()
    x[idx] = (0.5 + 0.4 / G * (torch.rand(8, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5)).float().double()
    v, t = _cube_mesh((0.36, 0.36, 0.36), (0.64, 0.64, 0.64))
    model = _model(const, [dict(type="mesh", verts=v, tris=t, resolution=24, surface="sticky", velocity=list(vc))])
    fc = model.field_colliders[0]
    assert isinstance(fc.source, MeshCollider) and fc.phi.is_cuda and fc.phi.dtype == torch.float32
    base, _, _ = om._stencil(const, x[idx])
    off, _ = om._offsets(torch.float64)
    nodes = ((base[:, None, :] + off[None]).double() / G).reshape(-1, 3)
    inside, phi, _ = xc.field_phi_normal(fc, nodes)
    assert bool(inside.all()) and float(phi.max()) < -0.02
    st = build_statics(model, vol, rho, clip, en, dev())
    _, outs = _gpu_step(model, st, (x,) + tuple(ins[1:]))
    vn = outs[1].detach().cpu().double()[idx]
    if not any(vc):
        assert torch.equal(vn, torch.zeros_like(vn))
    else:
        assert rel_max(vn, torch.tensor(vc, dtype=torch.float64).expand_as(vn)) < 4e-6


def test_grid_tape_with_a_field_collider_matches_recompute():
    from neuma_amd.sim import MPMCacheDiffSim
    const, (vol, rho, clip, en), ins, _ = fcc.mpm_grid(4096, 32, "noslip")
    res = {}
    for tag, cache in (("recompute", 0), ("auto", "auto"), ("overflow", 1)):
        model = _model(const, [Sphere(center=(0.5, 0.5, 0.5), radius=0.12, surface="slip"), fcc.collider("torus", "odd", "friction")])
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
            assert rel_max(g, r) < 1.5e-6, tag      # the bound of test_grid_tape_with_a_collider_matches_recompute


def test_an_empty_field_list_is_bitwise_the_model_without_colliders():
    """set_colliders([]) after a mesh collider: the same launches as ever, bitwise the same outputs and gradients (100 particles:
    one scatter workgroup, see test_an_empty_collider_list_is_bitwise_the_model_without_colliders)"""
    from gpu_util import mpm_case
    from neuma_amd.sim import MPMModelBuilder
    const, vol, rho, clip, en, x, v, C_, F, S = mpm_case(N=100, G=16, near_wall=False)
    ins = (x, v, C_, F, S)
    cfg = dict(gravity=list(const.gravity), bc=const.bc, num_grids=const.num_grids, dt=const.dt, bound=const.bound, eps=const.eps)
    torch.manual_seed(5)
    gws, res = None, []
    for kind in ("fresh", "emptied"):
        model = MPMModelBuilder().parse_cfg(cfg).finalize(dev(), requires_grad=True)
        st = build_statics(model, vol, rho, clip, en, dev())
        if kind == "emptied":
            model.set_colliders([fcc.collider("torus", "dyadic", "sticky")])
            _, changed = _gpu_step(model, st, ins)
            model.set_colliders([])
        assert model.colliders == [] and model.field_colliders == []
        gin, outs = _gpu_step(model, st, ins)
        gws = gws or [torch.randn(o.shape, device=dev()) for o in outs]
        grads = torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gws)), gin)
        res.append([t.detach().clone() for t in outs] + list(grads) + list(model.grid_export()))
        if kind == "emptied":
            assert not torch.equal(changed[1], outs[1])          # (the collider did act before it was removed)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_forward_sim_moves_a_mesh_collider():
    from neuma_amd.sim import MPMForwardSim, MPMModelBuilder
    const, (vol, rho, clip, en), ins, _ = fcc.mpm_grid(3001, 16, "freeslip")
    vel = [0.0, 0.5, 0.25]
    v, t = fcc.mesh("box")
    cfg = dict(gravity=list(const.gravity), bc=const.bc, num_grids=const.num_grids, dt=const.dt, bound=const.bound, eps=const.eps,
               colliders=[dict(type="plane", point=[0.5, 0.32, 0.5], normal=[0.2, 1, 0], surface="friction", friction=0.4),
                          dict(type="mesh", verts=v, tris=t, resolution=20, surface="slip", velocity=vel),
                          dict(type="mesh", verts=fcc.mesh("torus")[0], tris=fcc.mesh("torus")[1], resolution=20, surface="sticky")])
    model = MPMModelBuilder().parse_cfg(cfg).finalize(dev())
    assert len(model.colliders) == 1 and len(model.field_colliders) == 2
    o0, o1 = model.field_colliders[0].origin, model.field_colliders[1].origin
    phi0 = model.field_colliders[0].phi
    st = build_statics(model, vol, rho, clip, en, dev())
    state = model.state(3001)
    state.from_torch(**{k: t_.float().to(dev()) for k, t_ in zip(("x", "v", "C", "F", "stress"), ins)})
    sim = MPMForwardSim(model)
    for _ in range(20):
        outs = sim(st, state)
        model.step_colliders()
    assert all(bool(torch.isfinite(t_).all()) for t_ in outs)
    for a, c0, vv in zip(model.field_colliders[0].origin, o0, vel):
        assert abs(a - (c0 + 20 * const.dt * vv)) < 1e-15
    assert model.field_colliders[1].origin == o1 and model.colliders[0].point == (0.5, 0.32, 0.5)
    assert model.field_colliders[0].phi.data_ptr() == phi0.data_ptr()          # the field is built once and moved, not rebuilt


def test_every_other_path_refuses_field_colliders():
    from neuma_amd import _lib as L
    from neuma_amd import NeumaHipError
    const, (vol, rho, clip, en), ins, _ = fcc.mpm_grid(3001, 16, "noslip")
    model = _model(const, [fcc.collider("torus", "dyadic", "sticky")])
    st = build_statics(model, vol, rho, clip, en, dev())
    state = model.state(3001)
    state.from_torch(**{k: t.float().to(dev()) for k, t in zip(("x", "v", "C", "F", "stress"), ins)})
    lib, h = L.lib(), model.handle()
    msg = b"colliders: per-operator path only"
    cfg = L.nm_rollout_cfg(1, 1e-3, 0, 0, 0, None, None, 0, 0)
    cst, cur, w = st.c_struct(), state.particle.c_struct(), L.nm_mlp(None, None, None)
    buf = torch.zeros(64, device=dev())
    p = L.ptr(buf)
    for call in (lambda: lib.nm_rollout_forward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, None, 0, None),
                 lambda: lib.nm_rollout_backward(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, p, p, p, p, None, 0, None),
                 lambda: lib.nm_rollout_forward_sharded(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, None, 0, None,
                                                        1, 1, None, 0, None),
                 lambda: lib.nm_rollout_backward_sharded(h, 3001, C.byref(cfg), C.byref(cst), C.byref(w), C.byref(w), p, None, p, p, p, p,
                                                         None, 0, None, 1, 1, None, 0, None),
                 lambda: lib.nm_mpm_p2g(h, 3001, C.byref(cst), C.byref(cur), None),
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
    phi = model.field_colliders[0].phi

    def one(**kw):
        c = L.nm_field_collider(0, 0.0, (C.c_float * 3)(), (C.c_float * 3)(0.1, 0.1, 0.1), 0.05, (C.c_int32 * 3)(*phi.shape), phi.data_ptr())
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    assert lib.nm_mpm_set_field_colliders(h, 1, C.byref(one())) == 0
    for field, kw in (("surface", dict(surface=5)), ("friction", dict(friction=-0.5)), ("origin", dict(origin=(C.c_float * 3)(0.1, float("nan"), 0.1))),
                      ("velocity", dict(velocity=(C.c_float * 3)(0.0, float("inf"), 0.0))), ("spacing", dict(spacing=0.0)),
                      ("spacing", dict(spacing=-1.0)), ("dims", dict(dims=(C.c_int32 * 3)(1, 5, 5))),
                      ("dims", dict(dims=(C.c_int32 * 3)(1 << 10, 1 << 10, 1 << 8))), ("phi", dict(phi=None))):
        assert lib.nm_mpm_set_field_colliders(h, 1, C.byref(one(**kw))) == -1 and field.encode() in lib.nm_last_error(), field
    assert lib.nm_mpm_set_field_colliders(h, 5, C.byref(one())) == -1 and b"outside 0..4" in lib.nm_last_error()
    assert lib.nm_mpm_set_field_colliders(h, -1, None) == -1
    with pytest.raises(NeumaHipError, match="colliders: per-operator path only"):                       # still set
        model.forward_extra(st, state, st, state)
    model.set_colliders([])
    model.forward_extra(st, state, st, state)                      # and accepted again once they are gone
    # the training drivers refuse a config with a mesh entry by name
    from neuma_amd.sim.colliders import refuse_in_training
    with pytest.raises(NotImplementedError, match=r"sim\.colliders"):
        refuse_in_training({"sim": {"colliders": [dict(type="mesh", path="bowl.obj")]}}, "python -m neuma_amd.pretrain")


def test_inference_entry_point_with_a_mesh_collider(tmp_path, capsys):
    """`python -m neuma_amd.inference` on the two-object scene of test_inference_entry_point_with_a_plane_collider, with a sticky
    cuboid MESH (an .obj written here, scaled and translated by the entry) around the lower body in place of the half-space: the
    description is printed, the lower body never moves, the upper one falls."""
    import shutil
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

    G, steps = 32, 6
    # the unit cube [-1, 1]^3 as an .obj; scale 0.45 about the origin, then moved: x, z in 0.05 .. 0.95.  The lower body's stencil
    # nodes span 5 .. 12 cells in y; the cuboid must hold them and none of the upper body's (>= 18 cells): a second, flatter
    # entry would need a non-uniform scale, so the mesh itself is flat: y in +-0.46 -> 0.25 +- 0.207 = 1.4 .. 14.6 cells
    v, t = _cube_mesh((-1.0, -0.46, -1.0), (1.0, 0.46, 1.0))
    mesh_path = tmp_path / "slab.obj"
    cases.write_obj(mesh_path, v, t)
    colliders = [dict(type="sphere", center=[0.1, 0.9, 0.1], radius=0.04, surface="slip", velocity=[0.5, 0, 0]),
                 dict(type="mesh", path=str(mesh_path), scale=0.45, translate=[0.5, 0.25, 0.5], resolution=32, surface="sticky")]
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=colliders),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "mesh-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    capsys.readouterr()
    inference_main(["-c", str(demo), "-s", str(steps), "-vn", "mesh", "-dv", "r_0", "-sp", "mesh", "--draw_colliders",
                    "--result_root", str(tmp_path / "results")])
    out = capsys.readouterr().out
    assert "colliders: 1 (drawn in renders)" in out
    assert "mesh colliders: 1 (mesh colliders are not drawn in renders)" in out
    assert f"[0] mesh path={mesh_path} triangles=12 lattice=" in out and "surface=sticky" in out
    st_root = tmp_path / "results" / "inference_states" / "states_mesh"
    xs = [nio.load_particles_ply(st_root / f"{i:03d}.ply") for i in range(1, steps + 1)]
    objects = [load_object(o, assets, steps, dev()) for o in load_config(demo).objects]
    n0, n1 = (o.init_data.num_particles for o in objects)
    assert xs[0].shape == (n0 + n1, 3) and all(np.isfinite(x).all() for x in xs)
    lower0, upper0 = np.asarray(objects[1].init_data.pos), np.asarray(objects[0].init_data.pos)
    assert lower0[:, 1].max() * G + 1.5 < 14.0 and lower0[:, 1].min() * G - 1.5 > 2.0 and upper0[:, 1].min() * G - 1.5 > 15.0
    assert all(np.array_equal(x[n0:], xs[0][n0:]) for x in xs[1:])                     # sticky, static: v = 0 exactly
    assert np.abs(xs[0][n0:] - lower0).max() < 1e-7                                     # (the start positions, rounded to fp32 once)
    assert xs[-1][:n0, 1].mean() < upper0[:, 1].mean() - 0.8 * steps * 1e-3 * 0.5       # the upper body falls freely (0.5 per unit time)
