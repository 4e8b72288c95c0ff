"""GPU: drawing mesh colliders in renders (k_field_cast / k_field_hide of csrc/nm_draw.hip, the trace of csrc/nm_field_ray.h,
neuma_amd/collider_draw.py cast_field / front_opacity_field / draw) against the fp64 definition neuma_amd/extras/mesh_draw.py on
the scenes of tests/mesh_draw_cases.py, the exact consequences (repeatability, n = 0, a moved collider, the analytic path
untouched), every validation message, and the inference entry point with --draw_mesh_colliders.

Bounds.  hit and the hidden flags are branches: outside the pixels / Gaussians whose fp64 decision margin is small (at most 2 % /
1 % of a case, asserted without a GPU in tests/test_mesh_draw_cpu.py) they match exactly.  t (relative) and shade (absolute) stay
within 4 x the distance of the same formulas evaluated in torch fp32 on the CPU from fp64 on that case, with a floor of 1e-6.
Measured values: profiles/mesh_draw_parity_table.md."""
import ctypes as C
import shutil
from dataclasses import replace

import numpy as np
import pytest
import torch
import yaml

import collider_draw_cases as cc
import mesh_draw_cases as mc
import mesh_sdf_cases as cases
from gpu_util import dev, parity

pytestmark = pytest.mark.gpu


def _cast(cam, colliders, styles, fields, field_styles, tr):
    from neuma_amd import collider_draw as CD
    t, shade, hit = CD.cast(cam, colliders, styles, tr, device=dev())
    return CD.cast_field(cam, fields, field_styles, t, shade, hit, len(colliders), tr)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_kernels_match_the_fp64_definition(case):
    from neuma_amd import collider_draw as CD
    e, name = mc.evaluated(case), "mesh draw " + mc.case_id(case)
    cam, fields = e["cam"].to(dev()), mc.on_device(e["fields"], dev())
    t, shade, hit = _cast(cam, e["colliders"], e["styles"], fields, e["field_styles"], e["to_render"])
    ok = ~e["unsure"]
    parity(name, "hit: mismatches outside the margins", int((hit.cpu() != e["hit"])[ok].sum()), 0)
    parity(name, "t: finite where fp64 hits, inf elsewhere (mismatches)", int((torch.isinf(t.cpu()) != (e["hit"] < 0))[ok].sum()), 0)
    parity(name, "t (rel)", cc.t_error(t, e["t"], e["hit"], ok), cc.bound(e["err_t"]), noise=e["err_t"])
    parity(name, "shade (abs)", float((shade.cpu().double() - e["shade"])[:, ok].abs().max()), cc.bound(e["err_shade"]), noise=e["err_shade"])
    # two calls give the same bits
    again = _cast(cam, e["colliders"], e["styles"], fields, e["field_styles"], e["to_render"])
    assert all(torch.equal(a, b) for a, b in zip(again, (t, shade, hit)))
    # hidden flags and the front opacities, behind the analytic pass
    means, opacity = e["means"].to(dev()), e["opacity"].to(dev())
    front, hid = CD.front_opacity(cam, e["colliders"], means, opacity, e["to_render"], want_hidden=True)
    before = hid.clone()
    front, hid = CD.front_opacity_field(cam, fields, means, front, e["to_render"], hidden=hid)
    keep = ~e["hidden_unsure"]
    parity(name, "hidden: mismatches outside the margins", int((hid.cpu().bool() != e["hidden"])[keep].sum()), 0)
    assert bool((hid >= before).all()) and (e["colliders"] or int(hid.sum()) > 10)          # merged: nothing un-hidden
    assert torch.equal(front, torch.where(hid.bool()[:, None], torch.zeros_like(opacity), opacity))
    only = CD.front_opacity_field(cam, fields, means, opacity.clone(), e["to_render"])          # without the flags
    assert torch.equal((only == 0)[:, 0] | before.bool(), hid.bool())


def test_n0_leaves_the_buffers_and_a_moved_collider_is_drawn_at_the_new_place():
    from neuma_amd import collider_draw as CD
    e = mc.evaluated(mc.COMBINED[0])
    cam, tr = e["cam"].to(dev()), e["to_render"]
    t, shade, hit = CD.cast(cam, e["colliders"], e["styles"], tr, device=dev())
    kept = [x.clone() for x in (t, shade, hit)]
    out = CD.cast_field(cam, [], [], t, shade, hit, len(e["colliders"]), tr)
    assert all(torch.equal(a, b) for a, b in zip(out, kept)) and out[0] is t
    means, opacity = e["means"].to(dev()), e["opacity"].to(dev())
    front, hid = CD.front_opacity(cam, e["colliders"], means, opacity, tr, want_hidden=True)
    f0, h0 = front.clone(), hid.clone()
    CD.front_opacity_field(cam, [], means, front, tr, hidden=hid)
    assert torch.equal(front, f0) and torch.equal(hid, h0)
    # a moving collider, advanced as the model advances it: the definition at the new origin
    c = replace(mc.field("torus", 24), velocity=(0.1, 0.25, -0.05)).advanced(0.5)
    cam = cc.camera((128, 80), "identity")
    st = CD.parse_mesh_styles([{}], 0)
    rt, rshade, rhit, unsure, _ = mc.cast_both(cam, [], [], [c], st, tr, margins=True)
    _, _, hit_old = _cast(cam.to(dev()), [], [], mc.on_device([mc.field("torus", 24)], dev()), st, tr)
    t, shade, hit = _cast(cam.to(dev()), [], [], mc.on_device([c], dev()), st, tr)
    assert float(unsure.float().mean()) <= 0.02 and int((hit.cpu() != rhit)[~unsure].sum()) == 0
    assert int(((hit >= 0) != (hit_old >= 0)).sum()) > 500
    rt32, rs32, _ = mc.cast_both(cam, [], [], [c], st, tr, dtype=torch.float32)
    e_t, e_s = cc.t_error(rt32, rt, rhit, ~unsure), float((rs32.double() - rshade)[:, ~unsure].abs().max())
    parity("mesh draw moved torus", "t (rel)", cc.t_error(t, rt, rhit, ~unsure), cc.bound(e_t), noise=e_t)
    parity("mesh draw moved torus", "shade (abs)", float((shade.cpu().double() - rshade)[:, ~unsure].abs().max()), cc.bound(e_s), noise=e_s)


def test_argument_validation_names_the_field():
    from neuma_amd import _lib as L, collider_draw as CD
    from neuma_amd.extras import collider_draw as X
    from neuma_amd.sim.colliders import pack_fields
    lib = L.lib()
    cam = cc.camera((67, 45), "identity", device=dev())
    fields = mc.on_device([mc.field("box", 24), mc.field("torus", 24)], dev())
    arr, sty = pack_fields(fields), CD._styles(CD.parse_mesh_styles([{}, {}], 0))
    cfg, inv = CD._cfg(cam), CD._vec(X.inverse_projection(cam).reshape(16), C.c_double)
    one, zero = CD._vec((1, 1, 1)), CD._vec((0, 0, 0))
    t = torch.full((45, 67), float("inf"), device=dev()); shade = torch.zeros(3, 45, 67, device=dev())
    hit = torch.full((45, 67), -1, dtype=torch.int32, device=dev())
    args = lambda **kw: [kw.get("cfg", C.byref(cfg)), kw.get("inv", inv), kw.get("a", one), kw.get("b", zero), kw.get("n", 2),
                         kw.get("arr", arr), kw.get("sty", sty), kw.get("base", 0), kw.get("t", L.ptr(t)), L.ptr(shade), L.ptr(hit), None]
    for kw, word in ((dict(t=None), b"t, shade and hit"), (dict(n=5), b"field colliders: n = 5 outside 0..4"), (dict(n=-1), b"outside 0..4"),
                     (dict(a=CD._vec((1, 0, 1))), b"map_a: a <= 0"), (dict(a=CD._vec((1, -2, 1))), b"map_a: a <= 0"),
                     (dict(b=CD._vec((0, float("nan"), 0))), b"map_b"), (dict(sty=None), b"styles"), (dict(arr=None), b"field colliders: NULL"),
                     (dict(inv=None), b"inv_proj"), (dict(base=-1), b"hit_base")):
        assert lib.nm_collider_cast_field(*args(**kw)) == -1 and word in lib.nm_last_error(), (kw, lib.nm_last_error())
    bad = CD._styles(CD.parse_mesh_styles([{}, {}], 0))
    bad[1].color = CD._vec((0.5, float("inf"), 0.5))
    assert lib.nm_collider_cast_field(*args(sty=bad)) == -1 and b"style 1: color" in lib.nm_last_error()
    nan_cfg = CD._cfg(cam)
    nan_cfg.campos = CD._vec((0.0, float("nan"), 0.0))
    assert lib.nm_collider_cast_field(*args(cfg=C.byref(nan_cfg))) == -1 and b"campos" in lib.nm_last_error()
    means = torch.zeros(10, 3, device=dev()); op = torch.ones(10, 1, device=dev())
    campos = CD._vec(cam.camera_center.cpu())
    hide = lambda a: lib.nm_collider_hide_field(campos, one, zero, 2, a, 10, L.ptr(means), L.ptr(op), None, None)
    # the checks of nm_mpm_set_field_colliders, in both calls
    for field, kw in (("surface", dict(surface=5)), ("friction", dict(friction=-0.5)), ("origin", dict(origin=(C.c_float * 3)(0.1, float("nan"), 0.1))),
                      ("velocity", dict(velocity=(C.c_float * 3)(0.0, float("inf"), 0.0))), ("spacing", dict(spacing=0.0)),
                      ("spacing", dict(spacing=-1.0)), ("dims", dict(dims=(C.c_int32 * 3)(1, 5, 5))),
                      ("dims", dict(dims=(C.c_int32 * 3)(1 << 10, 1 << 10, 1 << 8))), ("phi", dict(phi=None))):
        worse = pack_fields(fields)
        for k, val in kw.items():
            setattr(worse[1], k, val)
        word = f"field collider 1: {field}".encode()
        assert lib.nm_collider_cast_field(*args(arr=worse)) == -1 and word in lib.nm_last_error(), (field, lib.nm_last_error())
        assert hide(worse) == -1 and word in lib.nm_last_error(), (field, lib.nm_last_error())
    assert lib.nm_collider_hide_field(campos, one, zero, 5, arr, 10, L.ptr(means), L.ptr(op), None, None) == -1 and b"outside 0..4" in lib.nm_last_error()
    assert lib.nm_collider_hide_field(campos, CD._vec((0, 1, 1)), zero, 2, arr, 10, L.ptr(means), L.ptr(op), None, None) == -1
    assert b"map_a" in lib.nm_last_error()
    assert lib.nm_collider_hide_field(campos, one, zero, 2, arr, 10, None, L.ptr(op), None, None) == -1 and b"means3D" in lib.nm_last_error()
    assert lib.nm_collider_hide_field(campos, one, zero, 2, arr, -1, L.ptr(means), L.ptr(op), None, None) == -1 and b"k < 0" in lib.nm_last_error()
    # nothing was written by a refused call; n = 0 and k = 0 are valid
    assert bool(torch.isinf(t).all()) and bool((hit == -1).all()) and bool((op == 1).all())
    assert lib.nm_collider_cast_field(*args(n=0, arr=None, sty=None)) == 0
    assert lib.nm_collider_hide_field(campos, one, zero, 0, None, 10, L.ptr(means), L.ptr(op), None, None) == 0
    assert lib.nm_collider_hide_field(campos, one, zero, 2, arr, 0, None, None, None, None) == 0
    # the Python wrappers refuse what the kernels would misread
    with pytest.raises(ValueError, match="styles"):
        CD.cast_field(cam, fields, [], t, shade, hit, 0)
    with pytest.raises(ValueError, match="cast_field"):
        CD.cast_field(cam, fields, CD.parse_mesh_styles([{}, {}], 0), t.double(), shade, hit, 0)
    with pytest.raises(ValueError, match="opacity_front"):
        CD.front_opacity_field(cam, fields, means, op[:5])


def _body(K=3000, center=(0.5, 0.5, 0.3), seed=0):
    g = torch.Generator().manual_seed(seed)
    means = torch.tensor(center) + (0.04 * torch.randn(K, 3, generator=g)).clamp(-0.1, 0.1)
    s2 = 0.02 ** 2
    cov = torch.tensor([s2, 0.0, 0.0, s2, 0.0, s2]).repeat(K, 1)
    return tuple(x.to(dev()).contiguous() for x in (means, cov, torch.full((K, 1), 0.9), torch.rand(K, 1, 3, generator=g)))


def _render(cam, bg, body, opacity=None, mask=False):
    from neuma_amd.tune import diff_rasterization
    means, cov, opa, shs = body
    return diff_rasterization(means, None, None, cam, bg, 0, cov, opa if opacity is None else opacity, shs, force_mask_data=mask).detach()


def test_draw_with_fields_and_the_analytic_path_as_it_was():
    """draw(): without fields= the image is, bit for bit, the composition of the three analytic calls (what --draw_colliders alone
    runs, mesh entry or not); with a field in front of the body the body's pixels show the field's shade, a field behind Gaussians
    hides none of them, and pixels that no collider hits keep img_all bit for bit."""
    from neuma_amd import collider_draw as CD
    from neuma_amd.sim.colliders import Sphere
    cam = cc.Camera(128, 80, (0.5, 0.5, 2.6), (0.5, 0.5, 0.5), fov_deg=40.0, device=dev())
    body = _body()
    means, _, opa, _ = body
    white = torch.ones(3, device=dev())
    img_all = _render(cam, white, body)
    front = lambda op, bg0: (_render(cam, bg0, body, op), _render(cam, bg0, body, op, mask=True))
    ball, style = [Sphere(center=(0.8, 0.75, 0.5), radius=0.12)], [CD.Style((0.9, 0.3, 0.2), 0.0)]
    t, shade, hit = CD.cast(cam, ball, style, device=dev())
    rgb_front, a_front = front(CD.front_opacity(cam, ball, means, opa), torch.zeros(3, device=dev()))
    today = CD.compose(cam, img_all, rgb_front, a_front, shade, hit)
    assert torch.equal(CD.draw(img_all, cam, ball, style, CD.IDENTITY, front, means, opa), today)
    # the rotated box (centre (0.5, 0.3, 0.5)) lifted in front of the body: z + 0.35, y + 0.2
    near = mc.on_device([replace(mc.field("box", 24), origin=tuple(o + s for o, s in zip(mc.field("box", 24).origin, (0.0, 0.2, 0.35))))], dev())
    fst = CD.parse_mesh_styles([{}], 1)
    out = CD.draw(img_all, cam, ball, style, CD.IDENTITY, front, means, opa, fields=near, field_styles=fst)
    _, fshade, fhit = CD.cast_field(cam, near, fst, t.clone(), shade.clone(), hit.clone(), 1)
    assert int((fhit == 1).sum()) > 500 and int((fhit == 0).sum()) > 100
    assert torch.equal(out[:, fhit < 0], img_all[:, fhit < 0]) and torch.equal(out[:, fhit == 0], today[:, fhit == 0])
    op_f, hid = CD.front_opacity_field(cam, near, means, CD.front_opacity(cam, ball, means, opa), hidden=torch.zeros(len(means), dtype=torch.uint8, device=dev()))
    assert float(hid.float().mean()) > 0.5
    # a body pixel that only hidden Gaussians touch (a_front = 0 exactly, in any render of these opacities) shows the field's shade
    a2 = front(op_f, torch.zeros(3, device=dev()))[1]
    gone = (img_all != 1).any(0) & (fhit == 1) & (a2[0] == 0)
    assert int(gone.sum()) > 50 and float((out - fshade)[:, gone].abs().max()) <= 1e-6
    far = mc.on_device([replace(mc.field("box", 24), origin=tuple(o + s for o, s in zip(mc.field("box", 24).origin, (0.0, 0.2, -0.35))))], dev())
    ahead = (means + torch.tensor([0.0, 0.0, 0.4], device=dev())).contiguous()          # the body's centres moved clear of the far box
    op2, hid2 = CD.front_opacity_field(cam, far, ahead, opa.clone(), hidden=torch.zeros(len(means), dtype=torch.uint8, device=dev()))
    assert not bool(hid2.any()) and torch.equal(op2, opa)
    only = CD.draw(img_all, cam, [], [], CD.IDENTITY, front, means, opa, fields=far, field_styles=CD.parse_mesh_styles([{}], 0))
    _, _, bhit = _cast(cam, [], [], far, CD.parse_mesh_styles([{}], 0), CD.IDENTITY)
    assert int((bhit == 0).sum()) > 300 and torch.equal(only[:, bhit < 0], img_all[:, bhit < 0])
    assert bool((only[:, bhit == 0] != img_all[:, bhit == 0]).any())


def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB")).astype(np.int32)


def test_inference_entry_point_draws_the_mesh_collider(tmp_path, capsys):
    """The two-object scene of test_gpu_field_colliders.py::test_inference_entry_point_with_a_mesh_collider with the sticky slab
    mesh as its only collider.  --draw_colliders alone: today's lines, and frames equal to the undrawn run's (nothing analytic to
    draw).  --draw_mesh_colliders (it implies the former; also as `sim.draw_mesh_colliders`): the new line, and frames that
    differ from the undrawn ones exactly on the pixels the field cast hits."""
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import collider_draw as CD, synth
    from neuma_amd.config import load_config
    from neuma_amd.dataset import CameraDataset
    from neuma_amd.inference import main as inference_main
    from neuma_amd.sim.colliders import parse_colliders
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

    G, steps = 32, 1
    v = np.array([(x, y, z) for x in (-1.0, 1.0) for y in (-0.46, 0.46) for z in (-1.0, 1.0)], dtype=np.float64)
    t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], dtype=np.int64)
    mesh_path = tmp_path / "slab.obj"
    cases.write_obj(mesh_path, v, cases._outward(v, t))
    colliders = [dict(type="mesh", path=str(mesh_path), scale=0.45, translate=[0.5, 0.25, 0.5], resolution=32, surface="sticky",
                      color=[0.2, 0.6, 0.3])]
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=colliders),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "mesh-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    results = tmp_path / "results"
    common = ["-c", str(demo), "-s", str(steps), "-dv", "r_0", "--result_root", str(results)]
    capsys.readouterr()
    inference_main(common + ["-vn", "plain"])
    out = capsys.readouterr().out
    assert "mesh colliders: 1\n" in out and "drawn" not in out
    inference_main(common + ["-vn", "analytic", "--draw_colliders"])
    out = capsys.readouterr().out
    assert "mesh colliders: 1 (mesh colliders are not drawn in renders)" in out and "(drawn in renders)" not in out
    assert out.count("draw_colliders: sim.colliders is empty, nothing to draw") == 1
    inference_main(common + ["-vn", "drawn", "--draw_mesh_colliders"])
    out = capsys.readouterr().out
    assert "mesh colliders: 1 (drawn in renders)" in out and "not drawn" not in out and "nothing to draw" not in out
    assert f"[0] mesh path={mesh_path} triangles=12 lattice=" in out
    c = load_config(demo)
    c.video_data.device = str(dev())
    ds = CameraDataset(c.video_data)
    cam = ds.getCameras("r_0", ds.steps[0])
    field = parse_colliders(colliders)[0].build(dev())
    style = CD.parse_mesh_styles(colliders, 0)
    assert style[0].color == (0.2, 0.6, 0.3)
    _, shade, hit = _cast(cam, [], [], [field], style, CD.IDENTITY)
    hit, shade = hit.cpu().numpy(), shade.cpu().numpy()
    assert (hit == 0).sum() > 200 and (hit < 0).sum() > 200
    roots = {n: results / "inference" / f"images_{n}" for n in ("plain", "analytic", "drawn")}
    for step in range(steps + 1):
        a, b, d = (_png(roots[n] / f"r_0_{step:03d}.png") for n in ("plain", "analytic", "drawn"))
        # (frame 0 is the un-deformed scene: bit for bit; two roll-outs differ by the order of the scatters' float atomics, one 8-bit level)
        tol = 0 if step == 0 else 1
        assert np.abs(a - b).max() <= tol                                       # --draw_colliders alone: the undrawn frames
        assert np.abs(a - d)[hit < 0].max() <= tol                              # elsewhere: img_all
        differs = (a != d).any(-1)
        # every hit pixel changed, but for those a body in front of the collider covers (not the white background undrawn)
        assert differs[hit >= 0].mean() > 0.8 and (differs | (a < 255).any(-1))[hit >= 0].all()
    # where nothing of a body is in front, the pixel is the cast's shade (8-bit)
    d0, a0 = _png(roots["drawn"] / "r_0_000.png"), _png(roots["plain"] / "r_0_000.png")
    bare = (hit == 0) & (a0 == 255).all(-1)
    assert bare.sum() > 100 and np.abs(d0[bare] - np.clip(shade.transpose(1, 2, 0)[bare] * 255.0, 0, 255)).max() <= 1.0
    # the key in the config does what the flag does
    cfg["sim"]["draw_mesh_colliders"] = True
    keyed = tmp_path / "keyed-tiny.yaml"
    keyed.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(keyed), "-s", "1", "-dv", "r_0", "--result_root", str(results), "-vn", "keyed"])
    assert "mesh colliders: 1 (drawn in renders)" in capsys.readouterr().out
    assert np.array_equal(_png(results / "inference" / "images_keyed" / "r_0_000.png"), d0)
