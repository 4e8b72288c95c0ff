"""CPU: the definition of drawing mesh colliders (neuma_amd/extras/mesh_draw.py) on the scenes of tests/mesh_draw_cases.py - its
behaviour (against the analytic sphere, the no-overshoot comparison that fixed step factor 1, ties, the cube-face hit, the camera
inside), the size of the unsure set, fp32 against fp64 outside it, and the parsing / printing around the new option.

The unsure set comes from fp64 margins only (extras/mesh_draw.py: grazing hits, near misses, rays at the step cap, t next to a
competing collider's, a Gaussian at the end of its segment or on the surface; plus the branches of the interval: a nearly empty
one, phi(t0) next to 0, two entries next to each other).  Cap: 2 % of the pixels and 1 % of the Gaussians of any case."""
from dataclasses import replace

import pytest
import torch

import collider_draw_cases as cc
import mesh_draw_cases as mc
from neuma_amd import collider_draw as CD
from neuma_amd.extras import collider_draw as X
from neuma_amd.extras import mesh_draw as XM
from neuma_amd.sim.colliders import FieldCollider, Sphere, describe_fields

PIXEL_CAP, GAUSSIAN_CAP = 0.02, 0.01


def _rays(cam, tr, dtype=torch.float64):
    o = X.sim_origin(X.ray_basis(cam)[1], tr).to(dtype)
    a = torch.tensor([float(v) for v in tr[0]], dtype=dtype)
    return o, X.pixel_dirs(cam, dtype) / a


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_unsure_set_is_small_and_fp32_decides_like_fp64_outside_it(case):
    e = mc.evaluated(case)
    assert float(e["unsure"].float().mean()) <= PIXEL_CAP and float(e["hidden_unsure"].float().mean()) <= GAUSSIAN_CAP
    ok, keep = ~e["unsure"], ~e["hidden_unsure"]
    assert int((e["hit32"] != e["hit"])[ok].sum()) == 0
    assert int((e["hidden32"] != e["hidden"])[keep].sum()) == 0
    n_field = int((e["hit"] >= len(e["colliders"])).sum())
    assert n_field > 100 and int(e["hidden"].sum()) > 30          # the fields are in view (also behind the analytic set) and hide Gaussians
    assert bool(torch.isfinite(e["t"][e["hit"] >= 0]).all()) and bool(torch.isinf(e["t"][e["hit"] < 0]).all())
    # the prototype's orientation figures: fp32 within about 1e-6 of fp64 in t, a few 1e-5 in the shade
    assert e["err_t"] < 5e-6 and e["err_shade"] < 2e-4


def test_sphere_field_agrees_with_the_analytic_sphere_within_a_spacing():
    """sphere320 is inscribed in the sphere of radius 0.3: its faces (circumradius 0.058) sag up to 0.0057 under it, which along a ray
    of incidence cosine c is 0.0057 / c.  At resolution 24 the spacing is 0.025: where the ray meets the sphere at c >= 0.5 the sag
    is under half a spacing, and with the interpolant's own error the two t differ by less than one spacing along the ray.  (At the
    silhouette the polyhedron and the sphere differ by more than that whatever the lattice.)"""
    c = mc.field("sphere320", 24)
    ball = Sphere(center=(0.5, 0.45, 0.55), radius=0.3)
    for size in cc.SIZES:
        for mp, tr in cc.MAPS.items():
            cam = cc.camera(size, mp)
            ta, _, hita = X.cast(cam, [ball], [CD.Style((1.0, 1.0, 1.0))], tr)
            t, _, hit = mc.cast_both(cam, [], [], [c], [CD.Style((1.0, 1.0, 1.0))], tr)
            o, ds = _rays(cam, tr)
            ds = ds.reshape(*ta.shape, 3)
            p = o + ta[..., None] * ds
            n = (p - torch.tensor(ball.center, dtype=torch.float64)) / ball.radius
            cos = -(n * ds).sum(-1) / ds.norm(dim=-1)
            m = (hita == 0) & (cos >= 0.5)
            assert int(m.sum()) > 150 and bool((hit[m] == 0).all())
            # t is the render-space distance: times L = |d_s| it is the distance along the ray in simulation units, the spacing's
            assert float(((t - ta)[m].abs() * ds.norm(dim=-1)[m]).max()) < c.spacing


@pytest.mark.parametrize("mesh", mc.MESHES)
@pytest.mark.parametrize("resolution", mc.RESOLUTIONS)
def test_step_factor_one_never_steps_past_the_first_root(mesh, resolution):
    """The comparison that chose step factor 1: a march with 1/8 of the step and 2000 steps finds the first root; the definition's
    march (factor 1, 192 steps) stops at the same one on every ray that does not run into its step cap - never on a later one,
    never on none.  phi is an interpolant, not an exact distance, so the stop may lie a little behind the fine one: within a tenth
    of a spacing along the ray, far below one cell, the smallest feature the lattice can hold.  Both cameras, maps and sizes."""
    c = mc.field(mesh, resolution)
    for size in cc.SIZES:
        for mp, tr in cc.MAPS.items():
            o, ds = _rays(cc.camera(size, mp), tr)
            cap = torch.full((ds.shape[0],), float("inf"), dtype=torch.float64)
            hc, tc, _, _, ic = XM.trace(c, o, ds, cap, want_n=False, info=True)
            hf, tf, _, _, fi = XM.trace(c, o, ds, cap, want_n=False, step_factor=0.125, max_steps=2000, info=True)
            free = (ic["steps"] < XM.STEPS) & (fi["steps"] < 2000)
            assert int((~free).sum()) <= 0.001 * free.numel()
            assert bool((hc == hf)[free].all()) and int(hf.sum()) > 100
            both = hc & hf
            assert float((((tc - tf) * ic["L"])[both]).max()) < 0.1 * c.spacing
            mean_steps = float(ic["steps"][hc].float().mean())
            assert 5.0 < mean_steps < 20.0, mean_steps


def test_ties_go_to_the_analytic_collider_and_to_the_first_field():
    """A field whose t equals what is in the buffer does not replace it: the buffer of its own cast, fed back, stays bit for bit -
    for an analytic owner (hit index 0) and for a field listed twice (the first keeps the pixel)."""
    c, st = mc.field("box", 24), [CD.Style((0.2, 0.4, 0.6))]
    cam, tr = cc.camera((67, 45), "identity"), cc.MAPS["identity"]
    empty = X.cast(cam, [], [], tr)
    t, shade, hit = XM.cast_field(cam, [c], st, tr, *empty, hit_base=1)
    assert int((hit == 1).sum()) > 100
    owned = torch.where(hit == 1, torch.zeros_like(hit), hit)          # as if analytic collider 0 had written exactly these t
    t2, shade2, hit2 = XM.cast_field(cam, [c], [CD.Style((0.9, 0.9, 0.9))], tr, t, shade, owned, hit_base=1)
    assert torch.equal(t2, t) and torch.equal(shade2, shade) and torch.equal(hit2, owned)
    t3, shade3, hit3 = XM.cast_field(cam, [c, c], [st[0], CD.Style((0.9, 0.9, 0.9))], tr, *empty, hit_base=0)
    assert torch.equal(t3, t) and torch.equal(shade3, shade) and not bool((hit3 == 1).any()) and int((hit3 == 0).sum()) == int((hit == 1).sum())


def test_cube_face_hit_carries_the_cube_faces_normal():
    """The pushed icosahedron is cut by the cube's face x = 1, which the camera (x = 1.7) sees: those pixels hit at the cube's entry
    with the normal +x, i.e. the shade of a +x face under the headlight."""
    e = mc.evaluated(mc.PUSHED[1])
    cam, tr = e["cam"], e["to_render"]
    o, ds = _rays(cam, tr)
    hit, t, which, n = XM.trace(e["fields"][0], o, ds, torch.full((ds.shape[0],), float("inf"), dtype=torch.float64))
    face = hit & (which == 0)
    assert int(face.sum()) > 100 and int((hit & (which == 6)).sum()) > 100 and not bool((hit & (which > 0) & (which < 6)).any())
    assert bool((n[face] == torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)).all())
    p = o + t[face, None] * ds[face]
    assert float((p[:, 0] - 1.0).abs().max()) < 1e-12
    col = torch.tensor(e["field_styles"][0].color, dtype=torch.float64)
    dr = X.pixel_dirs(cam)[face]
    expect = col[:, None] * (0.35 + 0.65 * torch.clamp(-dr[:, 0], min=0.0))[None]
    assert float((e["shade"].reshape(3, -1)[:, face] - expect).abs().max()) < 1e-12


def test_camera_inside_the_solid_faces_the_camera():
    c = mc.field("box", 24)
    eye = (0.5, 0.3, 0.5)                                                   # the box's centre
    cam = cc.Camera(67, 45, eye, (0.9, 0.5, 0.6), fov_deg=38.0)
    st = [CD.Style((0.2, 0.5, 0.8))]
    t, shade, hit = mc.cast_both(cam, [], [], [c], st, X.IDENTITY)
    assert bool((hit == 0).all()) and bool((t == 0).all())
    assert float((shade - torch.tensor(st[0].color, dtype=torch.float64)[:, None, None]).abs().max()) < 1e-15          # n . l = 1
    g = torch.tensor([[0.9, 0.5, 0.6], [0.52, 0.31, 0.5]])
    assert XM.hidden_field(torch.tensor(eye), [c], g).tolist() == [True, True]


def test_hidden_by_the_segment_or_by_the_mean_inside():
    c = mc.field("box", 24)          # the rotated box around (0.5, 0.3, 0.5)
    eye = torch.tensor([1.7, 1.25, 2.0])
    behind = 2 * torch.tensor([0.5, 0.3, 0.5]) - eye
    g = torch.stack([torch.tensor([0.5, 0.3, 0.5]), behind, torch.tensor([0.5, 0.9, 0.5]), eye + 0.3 * (torch.tensor([0.5, 0.3, 0.5]) - eye)])
    assert XM.hidden_field(eye, [c], g).tolist() == [True, True, False, False]
    assert XM.hidden_field(eye, [c], g, hidden=torch.tensor([False, False, True, False])).tolist() == [True, True, True, False]
    op = torch.full((4, 1), 0.5)
    cam = cc.Camera(8, 8, eye.tolist(), (0.5, 0.3, 0.5))
    out, hid = CD.front_opacity_field(cam, [c], g, op, hidden=torch.zeros(4, dtype=torch.uint8))
    assert out[:, 0].tolist() == [0.0, 0.0, 0.5, 0.5] and hid.tolist() == [1, 1, 0, 0]


def test_a_moved_field_is_drawn_at_the_new_place_and_n0_is_the_identity():
    c = replace(mc.field("torus", 24), velocity=(0.0, 0.25, 0.0))
    cam, tr, st = cc.camera((67, 45), "identity"), X.IDENTITY, [CD.Style((0.5, 0.5, 0.5))]
    base = X.cast(cam, [], [], tr)
    _, _, hit0 = XM.cast_field(cam, [c], st, tr, *base)
    moved = c.advanced(0.4)
    assert abs(moved.origin[1] - c.origin[1] - 0.1) < 1e-12 and moved.phi is c.phi
    _, _, hit1 = XM.cast_field(cam, [moved], st, tr, *base)
    # the image moves as that of an analytic sphere moved alike does (mean row of the hit pixels)
    balls = [X.cast(cam, [Sphere(center=(0.5, y, 0.5), radius=0.1)], st, tr)[2] for y in (0.4, 0.5)]
    rows = [float(torch.nonzero(h >= 0)[:, 0].float().mean()) for h in (hit0, hit1, *balls)]
    assert abs(rows[1] - rows[0]) > 3 and abs((rows[1] - rows[0]) - (rows[3] - rows[2])) < 1.0
    t, shade, hit = CD.cast_field(cam, [], [], base[0].float(), base[1].float(), base[2], 0, tr)
    assert torch.equal(t, base[0].float()) and torch.equal(hit, base[2])


def test_parse_mesh_styles():
    nodes = [dict(type="mesh", path="a.obj"), dict(type="mesh", path="b.obj", color=[0.1, 0.2, 0.3], checker=0.5)]
    st = CD.parse_mesh_styles(nodes, 3)
    assert st[0] == CD.Style(CD.PALETTE[3], 0.0) and st[1] == CD.Style((0.1, 0.2, 0.3), 0.0)          # by the index in the whole list
    assert CD.parse_mesh_styles(nodes, 7)[1 - 1].color == CD.PALETTE[7] and CD.parse_mesh_styles([nodes[0]], 8)[0].color == CD.PALETTE[0]
    assert CD.parse_mesh_styles(None) == [] and CD.parse_mesh_styles([FieldCollider(phi=torch.zeros(2, 2, 2), spacing=0.1, dims=(2, 2, 2))], 1)[0].color == CD.PALETTE[1]
    with pytest.raises(ValueError, match=r"collider 4: color: three numbers in 0\.\.1"):
        CD.parse_mesh_styles([nodes[0], dict(type="mesh", color=[0.1, 2.0, 0.3])], 3)
    with pytest.raises(ValueError, match="at most 4"):
        CD.parse_mesh_styles([{}] * 5)
    # parse_styles and its limit stay what they were
    assert len(CD.parse_styles([dict(type="sphere")] * 8)) == 8
    with pytest.raises(ValueError, match=r"outside 0\.\.8"):
        CD.parse_styles([dict(type="sphere")] * 9)


def test_option_parsing_and_the_start_up_line():
    from neuma_amd.evaluate import parse_args as render_args
    from neuma_amd.inference import parse_args as inference_args
    for parse in (inference_args, render_args):
        a = parse(["-c", "x.yaml", "-vn", "v", "--draw_mesh_colliders"])
        assert a.draw_mesh_colliders is True and a.draw_colliders is False
        assert parse(["-c", "x.yaml", "-vn", "v"]).draw_mesh_colliders is False
    assert CD.mesh_wanted({"draw_mesh_colliders": True}, None) and CD.mesh_wanted({}, {"draw_mesh_colliders": True})
    assert not CD.mesh_wanted({"draw_colliders": True}, {"draw_colliders": True}) and not CD.wanted({"draw_mesh_colliders": True}, {})
    f = [mc.field("box", 24)]
    assert describe_fields(f, drawn=True).splitlines()[0] == "mesh colliders: 1 (drawn in renders)"
    assert describe_fields(f, draw_wanted=True, drawn=True).splitlines()[0] == "mesh colliders: 1 (drawn in renders)"
    # its present outputs
    assert describe_fields(f).splitlines()[0] == "mesh colliders: 1"
    assert describe_fields(f, draw_wanted=True).splitlines()[0] == "mesh colliders: 1 (mesh colliders are not drawn in renders)"
    assert describe_fields(f, drawn=True).splitlines()[1:] == describe_fields(f).splitlines()[1:]
