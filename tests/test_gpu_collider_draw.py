"""GPU: drawing colliders in renders (csrc/nm_draw.hip, neuma_amd/collider_draw.py) - the three kernels against the fp64 definition
of neuma_amd/extras/collider_draw.py on the scenes of tests/collider_draw_cases.py, the pixel-ray convention against the
rasterizer, the consequences of the composition with real renders, and the two entry points with --draw_colliders.

Bounds.  hit and the hidden flags are branches: outside the pixels / Gaussians whose fp64 decision margin is small (at most 2 % /
1 % of a case, asserted without a GPU in tests/test_collider_draw_cpu.py) they match exactly.  t (relative) and shade (absolute)
stay within 4 x the distance of the same formulas evaluated in torch fp32 on the CPU from fp64, with a floor of 1e-6."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch
import yaml

import collider_draw_cases as cc
from gpu_util import dev, parity

pytestmark = pytest.mark.gpu


def _body(K=3000, center=(0.5, 0.5, 0.3), seed=0):
    """An opaque blob of K small isotropic Gaussians within 0.1 of `center`: means, cov6, opacity, degree-0 SH colours"""
    g = torch.Generator().manual_seed(seed)
    means = torch.tensor(center) + (0.04 * torch.randn(K, 3, generator=g)).clamp(-0.1, 0.1)
    s2 = 0.02 ** 2
    cov = torch.tensor([s2, 0.0, 0.0, s2, 0.0, s2]).repeat(K, 1)
    opa = torch.full((K, 1), 0.9)
    shs = torch.rand(K, 1, 3, generator=g)
    return tuple(t.to(dev()).contiguous() for t in (means, cov, opa, shs))


def _render(cam, bg, body, opacity=None, mask=False):
    from neuma_amd.tune import diff_rasterization
    means, cov, opa, shs = body
    return diff_rasterization(means, None, None, cam, bg, 0, cov, opa if opacity is None else opacity, shs, force_mask_data=mask).detach()


def _axis_camera(W=128, H=80):
    return cc.Camera(W, H, (0.5, 0.5, 2.6), (0.5, 0.5, 0.5), fov_deg=40.0, device=dev())


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_kernels_match_the_fp64_definition(case):
    from neuma_amd import collider_draw as CD
    from neuma_amd.extras import collider_draw as X
    e, name = cc.evaluated(case), cc.case_id(case)
    cam = e["cam"].to(dev())
    t, shade, hit = CD.cast(cam, e["colliders"], e["styles"], e["to_render"], device=dev())
    ok = ~e["unsure"]
    parity(name, "hit: mismatches outside the margins", int((hit.cpu() != e["hit"])[ok].sum()), 0)
    parity(name, "t: finite where fp64 hits, inf elsewhere (mismatches)", int((torch.isinf(t.cpu()) != (e["hit"] < 0))[ok].sum()), 0)
    parity(name, "t (rel)", cc.t_error(t, e["t"], e["hit"], ok), cc.bound(e["err_t"]), noise=e["err_t"])
    parity(name, "shade (abs)", float((shade.cpu().double() - e["shade"])[:, ok].abs().max()), cc.bound(e["err_shade"]), noise=e["err_shade"])
    # hidden flags and the front opacities
    means, opacity = e["means"].to(dev()), e["opacity"].to(dev())
    front, hid = CD.front_opacity(cam, e["colliders"], means, opacity, e["to_render"], want_hidden=True)
    keep = ~e["hidden_unsure"]
    parity(name, "hidden: mismatches outside the margins", int((hid.cpu().bool() != e["hidden"])[keep].sum()), 0)
    assert torch.equal(front, torch.where(hid.bool()[:, None], torch.zeros_like(opacity), opacity))
    assert torch.equal(CD.front_opacity(cam, e["colliders"], means, opacity, e["to_render"]), front)
    # the composed image, from this cast and random images
    g = torch.Generator().manual_seed(5)
    H, W = cam.image_height, cam.image_width
    img, rgb = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    alpha = torch.rand(3, H, W, generator=g)
    out = CD.compose(cam, img.to(dev()), rgb.to(dev()), alpha.to(dev()), shade, hit)
    sh_c, hit_c = shade.cpu(), hit.cpu()
    ref = X.compose(img.double(), rgb.double(), alpha[0].double(), sh_c.double(), hit_c)
    e32 = float((X.compose(img, rgb, alpha[0], sh_c, hit_c).double() - ref).abs().max())
    parity(name, "composed image (abs)", float((out.cpu().double() - ref).abs().max()), cc.bound(e32), noise=e32)
    assert torch.equal(out.cpu()[:, hit_c < 0], img[:, hit_c < 0])


def test_argument_validation_names_the_field():
    from neuma_amd import _lib as L, collider_draw as CD
    from neuma_amd.extras import collider_draw as X
    from neuma_amd.sim.colliders import pack, parse_colliders
    lib = L.lib()
    cam = cc.camera((67, 45), "identity", device=dev())
    cols = parse_colliders(cc.SETS["eight"])
    arr, sty = pack(cols), CD._styles(CD.parse_styles(cc.SETS["eight"]))
    cfg, inv = CD._cfg(cam), CD._vec(X.inverse_projection(cam).reshape(16), C.c_double)
    one, zero = CD._vec((1, 1, 1)), CD._vec((0, 0, 0))
    t = torch.zeros(45, 67, device=dev()); shade = torch.zeros(3, 45, 67, device=dev()); hit = torch.zeros(45, 67, dtype=torch.int32, device=dev())
    args = lambda **kw: [kw.get("cfg", C.byref(cfg)), kw.get("inv", inv), kw.get("a", one), kw.get("b", zero), kw.get("n", 8),
                         kw.get("arr", arr), kw.get("sty", sty), kw.get("t", L.ptr(t)), L.ptr(shade), L.ptr(hit), None]
    for kw, word in ((dict(t=None), b"t, shade and hit"), (dict(n=9), b"outside 0..8"), (dict(n=-1), b"outside 0..8"),
                     (dict(a=CD._vec((1, 0, 1))), b"map_a: a <= 0"), (dict(a=CD._vec((1, -2, 1))), b"map_a: a <= 0"),
                     (dict(b=CD._vec((0, float("nan"), 0))), b"map_b"), (dict(sty=None), b"styles"), (dict(arr=None), b"colliders"),
                     (dict(inv=None), b"inv_proj")):
        assert lib.nm_collider_cast(*args(**kw)) == -1 and word in lib.nm_last_error(), (kw, lib.nm_last_error())
    bad = CD._styles(CD.parse_styles(cc.SETS["eight"]))
    bad[2].color = CD._vec((0.5, float("inf"), 0.5))
    assert lib.nm_collider_cast(*args(sty=bad)) == -1 and b"style 2: color" in lib.nm_last_error()
    bad[2].color, bad[5].checker = CD._vec((0.5, 0.5, 0.5)), float("nan")
    assert lib.nm_collider_cast(*args(sty=bad)) == -1 and b"style 5: checker" in lib.nm_last_error()
    worse = pack(cols)
    worse[1].radius = -1.0
    assert lib.nm_collider_cast(*args(arr=worse)) == -1 and b"collider 1: radius" in lib.nm_last_error()
    m = torch.zeros(10, 3, device=dev()); op = torch.ones(10, 1, device=dev())
    campos = CD._vec(cam.camera_center.cpu())
    assert lib.nm_collider_hide(campos, one, zero, 9, arr, 10, L.ptr(m), L.ptr(op), L.ptr(op), None, None) == -1 and b"outside 0..8" in lib.nm_last_error()
    assert lib.nm_collider_hide(campos, CD._vec((0, 1, 1)), zero, 8, arr, 10, L.ptr(m), L.ptr(op), L.ptr(op), None, None) == -1
    assert b"map_a" in lib.nm_last_error()
    assert lib.nm_collider_hide(campos, one, zero, 8, arr, 10, L.ptr(m), None, L.ptr(op), None, None) == -1 and b"opacity" in lib.nm_last_error()
    assert lib.nm_collider_compose(C.byref(cfg), L.ptr(shade), L.ptr(shade), None, L.ptr(shade), L.ptr(hit), L.ptr(shade), None) == -1
    assert b"a_front" in lib.nm_last_error()
    # n = 0 is valid: no hits, nothing hidden
    t0, s0, h0 = CD.cast(cam, [], [], device=dev())
    assert bool(torch.isinf(t0).all()) and bool((s0 == 0).all()) and bool((h0 == -1).all())
    front, hid = CD.front_opacity(cam, [], m, op, want_hidden=True)
    assert torch.equal(front, op) and not bool(hid.any())


@pytest.mark.parametrize("principal", [(0.0, 0.0), (0.13, -0.09)], ids=["centred", "off-centre"])
def test_pixel_rays_follow_the_rasterizers_convention(principal):
    """One small opaque Gaussian at the centre of a sphere collider: the brightest pixel of its render and the pixel of smallest t
    of the sphere's cast coincide within one pixel - with the centred camera and with the off-centre principal point."""
    from neuma_amd import collider_draw as CD
    from neuma_amd.sim.colliders import Sphere
    cam = cc.Camera(128, 80, (1.7, 1.25, 2.0), (0.5, 0.45, 0.5), fov_deg=38.0, principal=principal, device=dev())
    centre = (0.3, 0.62, 0.4)
    s2 = 0.015 ** 2
    body = (torch.tensor([centre], device=dev()), torch.tensor([[s2, 0.0, 0.0, s2, 0.0, s2]], device=dev()),
            torch.full((1, 1), 0.99, device=dev()), torch.ones(1, 1, 3, device=dev()))
    img = _render(cam, torch.zeros(3, device=dev()), body)[0]
    assert float(img.max()) > 0.3
    by, bx = divmod(int(img.argmax()), cam.image_width)
    t, _, hit = CD.cast(cam, [Sphere(center=centre, radius=0.1)], [CD.Style((1.0, 1.0, 1.0), 0.0)], device=dev())
    ty, tx = divmod(int(t.argmin()), cam.image_width)
    assert int(hit[ty, tx]) == 0 and 5 < tx < 122 and 5 < ty < 74
    assert abs(tx - cam.image_width // 2) > 8 or abs(ty - cam.image_height // 2) > 8          # off the image centre: a shift would show
    parity(f"convention-{'off-centre' if principal[0] else 'centred'}", "brightest pixel vs nearest pixel (pixels)",
           max(abs(bx - tx), abs(by - ty)), 1)


def test_no_collider_and_missed_pixels_keep_the_image_bit_for_bit():
    from neuma_amd import collider_draw as CD
    from neuma_amd.sim.colliders import Sphere
    cam, body = _axis_camera(), _body()
    bg = torch.tensor([1.0, 0.9, 0.8], device=dev())
    img_all = _render(cam, bg, body)
    means, _, opa, _ = body
    front = lambda op, bg0: (_render(cam, bg0, body, op), _render(cam, bg0, body, op, mask=True))
    assert CD.draw(img_all, cam, [], [], CD.IDENTITY, front, means, opa) is img_all              # the drivers' path without colliders
    t, shade, hit = CD.cast(cam, [], [], device=dev())
    rgb_front, a_front = front(CD.front_opacity(cam, [], means, opa), torch.zeros(3, device=dev()))
    assert torch.equal(CD.compose(cam, img_all, rgb_front, a_front, shade, hit), img_all)          # and through the kernels with n = 0
    ball = [Sphere(center=(0.8, 0.75, 0.5), radius=0.12)]
    style = [CD.Style((0.9, 0.3, 0.2), 0.0)]
    out = CD.draw(img_all, cam, ball, style, CD.IDENTITY, front, means, opa)
    _, _, hit = CD.cast(cam, ball, style, device=dev())
    assert 100 < int((hit >= 0).sum()) < 2000
    assert torch.equal(out[:, hit < 0], img_all[:, hit < 0]) and bool((out[:, hit >= 0] != img_all[:, hit >= 0]).any())


def test_box_in_front_of_and_behind_the_body_and_a_stripe():
    from neuma_amd import collider_draw as CD
    from neuma_amd.sim.colliders import Box
    cam, body = _axis_camera(), _body()
    means, _, opa, _ = body
    white, black = torch.ones(3, device=dev()), torch.zeros(3, device=dev())
    front = lambda op, bg0: (_render(cam, bg0, body, op), _render(cam, bg0, body, op, mask=True))
    style = [CD.Style((0.3, 0.6, 0.9), 0.0)]
    # in front: every Gaussian is hidden, so the body's pixels show the box's shade
    near = [Box(center=(0.5, 0.5, 0.7), half=(0.3, 0.3, 0.05))]
    img_all = _render(cam, white, body)
    body_px = (img_all != 1).any(0)
    _, shade, hit = CD.cast(cam, near, style, device=dev())
    _, hid = CD.front_opacity(cam, near, means, opa, want_hidden=True)
    assert bool(hid.all()) and int(body_px.sum()) > 50 and bool((hit[body_px] == 0).all())
    out = CD.draw(img_all, cam, near, style, CD.IDENTITY, front, means, opa)
    parity("box-in-front", "body pixels vs the cast's shade (abs)", float((out - shade)[:, body_px].abs().max()), 1e-6)
    assert torch.equal(out[:, hit < 0], img_all[:, hit < 0])
    # behind, black background: nothing is hidden and the body keeps its pixels but for what shines through
    far = [Box(center=(0.5, 0.5, 0.1), half=(0.3, 0.3, 0.05))]
    img_all = _render(cam, black, body)
    op_front, hid = CD.front_opacity(cam, far, means, opa, want_hidden=True)
    assert not bool(hid.any()) and torch.equal(op_front, opa)
    rgb_front, a_front = front(op_front, black)
    _, shade, hit = CD.cast(cam, far, style, device=dev())
    out = CD.compose(cam, img_all, rgb_front, a_front, shade, hit)
    # (draw renders its own front images: two renders of one view agree to the order of their sums, not bit for bit)
    assert float((out - CD.draw(img_all, cam, far, style, CD.IDENTITY, front, means, opa)).abs().max()) < 1e-5
    excess = float(((out - img_all).abs() - (1.0 - a_front[0])[None]).max())
    parity("box-behind", "abs(out - img_all) - (1 - a_front), max", excess, 1e-6)
    assert float((out - img_all).abs().max()) > 0.2 and int(((a_front[0] > 0.5) & (hit >= 0)).sum()) > 50
    # a stripe: pixel rows outside [16 tile_y0, 16 tile_y1) stay as they were
    canvas = torch.full_like(out, 7.0)
    stripe = CD.compose(cam, img_all, rgb_front, a_front, shade, hit, tile_rows=(1, 3), out=canvas)
    assert stripe is canvas and torch.equal(stripe[:, 16:48], out[:, 16:48])
    assert bool((stripe[:, :16] == 7).all()) and bool((stripe[:, 48:] == 7).all())
    last = CD.compose(cam, img_all, rgb_front, a_front, shade, hit, tile_rows=(4, 9))            # clipped at the image's last row
    assert torch.equal(last[:, 64:], out[:, 64:]) and bool((last[:, :64] == 0).all())


def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB")).astype(np.int32)


def _hit_of_frame(cam, nodes, dt, step, to_render):
    """the cast's hit mask for the colliders as the drivers hold them at frame `step` (moving ones advanced once per step)"""
    from neuma_amd import collider_draw as CD
    from neuma_amd.sim.colliders import parse_colliders
    cols = parse_colliders(nodes)
    for _ in range(step):
        cols = [c.advanced(dt) if c.moving else c for c in cols]
    _, _, hit = CD.cast(cam, cols, CD.parse_styles(nodes), to_render, device=dev())
    return hit.cpu().numpy()


def test_inference_entry_point_draws_the_colliders(tmp_path, capsys):
    """The two-object collider scene of test_gpu_colliders.py::test_inference_entry_point_with_a_plane_collider (one body above a
    sticky half-space, the other wholly inside it, a moving sphere): without the flag the line and the images are today's; with
    --draw_colliders the line says so, the frames differ from the undrawn ones exactly on the cast's hit pixels, and the lower body
    is gone - the frame equals that of the scene without it."""
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import synth
    from neuma_amd.config import load_config
    from neuma_amd.dataset import CameraDataset
    from neuma_amd.inference import main as inference_main
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

    G, steps = 32, 2
    colliders = [dict(type="plane", point=[0.5, 14.6 / G, 0.5], normal=[0, 2, 0], surface="sticky"),
                 dict(type="sphere", center=[0.1, 0.9, 0.1], radius=0.04, surface="slip", velocity=[0.5, 0, 0])]
    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=G, eps=6e-7, colliders=colliders),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "colliders-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    results = tmp_path / "results"
    common = ["-c", str(demo), "-s", str(steps), "-dv", "r_0", "--result_root", str(results)]
    capsys.readouterr()
    inference_main(common + ["-vn", "plain"])
    assert "colliders: 2 (not drawn in renders)" in capsys.readouterr().out
    inference_main(common + ["-vn", "drawn", "--draw_colliders"])
    out = capsys.readouterr().out
    assert "colliders: 2 (drawn in renders)" in out and "not drawn" not in out
    assert "[0] plane point=(0.5, 0.45625, 0.5) normal=(0.0, 1.0, 0.0) surface=sticky" in out
    c = load_config(demo)
    c.video_data.device = str(dev())
    ds = CameraDataset(c.video_data)
    cam = ds.getCameras("r_0", ds.steps[0])
    plain_root, drawn_root = (results / "inference" / f"images_{n}" for n in ("plain", "drawn"))
    assert sorted(p.name for p in drawn_root.glob("*.png")) == [f"r_0_{i:03d}.png" for i in range(steps + 1)]
    for step in (0, steps):
        hit = _hit_of_frame(cam, colliders, float(base["sim"]["dt"]), step, ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
        a, b = _png(plain_root / f"r_0_{step:03d}.png"), _png(drawn_root / f"r_0_{step:03d}.png")
        differs = (a != b).any(-1)
        assert (hit == 0).sum() > 200 and (hit < 0).sum() > 200
        # (frame 0 is the un-deformed scene: bit for bit; two roll-outs differ by the order of the scatters' float atomics, one 8-bit level)
        assert np.abs(a - b)[hit < 0].max() <= (0 if step == 0 else 1)
        # every hit pixel changed, but for those a body in front of the collider covers (not the white background undrawn)
        assert differs[hit >= 0].mean() > 0.8 and (differs | (a < 255).any(-1))[hit >= 0].all()
    # the key in the config does what the flag does; the lower body, inside the half-space, is not visible: the scene without it
    # gives the same first frame
    cfg["sim"]["draw_colliders"] = True
    cfg["objects"] = cfg["objects"][:1]
    upper = tmp_path / "upper-tiny.yaml"
    upper.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(upper), "-s", "1", "-dv", "r_0", "--result_root", str(results), "-vn", "upper"])
    assert "(drawn in renders)" in capsys.readouterr().out
    a0, b0, u0 = (_png(results / "inference" / f"images_{n}" / "r_0_000.png") for n in ("plain", "drawn", "upper"))
    hit = _hit_of_frame(cam, colliders, 0.0, 0, ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    assert ((a0 < 250).any(-1) & (hit == 0)).sum() > 30                    # undrawn, the lower body shows where the half-space will be
    assert np.abs(b0 - u0).max() <= 1
    # the flag without colliders: one note, nothing drawn; objects with different alignments under denormalize: refused by name
    del cfg["sim"]["colliders"]
    none = tmp_path / "none-tiny.yaml"
    none.write_text(yaml.safe_dump(cfg, sort_keys=False))
    inference_main(["-c", str(none), "-s", "1", "-dv", "r_0", "--result_root", str(results), "-vn", "none"])
    text = capsys.readouterr().out
    assert text.count("draw_colliders: sim.colliders is empty, nothing to draw") == 1 and "drawn in renders" not in text
    with pytest.raises(ValueError, match="denormalize"):
        inference_main(_with_denormalize(tmp_path, demo) + ["-s", "1", "-dv", "r_0", "--result_root", str(results), "-vn", "mixed",
                                                            "--draw_colliders"])


def _with_denormalize(tmp_path, demo):
    cfg = yaml.safe_load(demo.read_text())
    cfg["denormalize"] = True
    path = tmp_path / "denorm-tiny.yaml"
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    return ["-c", str(path)]


def test_render_entry_point_draws_the_colliders_under_its_map(tmp_path, capsys):
    """`python -m neuma_amd.render --draw_colliders` on the single-object experiment writer, with sim_bounds that make the
    simulation -> render map a per-axis one: the frames differ from the undrawn ones exactly on the cast's hit pixels."""
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import collider_draw as CD
    from neuma_amd.config import load_config
    from neuma_amd.dataset import CameraDataset
    from neuma_amd.evaluate import main as render_main
    from neuma_amd.finetune import particle_init_data
    path, _ = _write_experiment(tmp_path, frames=1)
    cfg = yaml.safe_load(path.read_text())
    cfg["particle_data"]["shape"]["sim_bounds"] = [[0.2, 0.3, 0.25], [0.8, 0.9, 0.75]]
    nodes = [dict(type="plane", point=[0.5, 0.36, 0.5], normal=[0.1, 1, 0], surface="friction", friction=0.3, checker=0.1),
             dict(type="box", center=[0.68, 0.62, 0.36], half=[0.04, 0.08, 0.05], euler_xyz_deg=[0, 30, 10], surface="slip")]
    cfg["sim"] = dict(cfg["sim"], eps=6e-7, colliders=nodes)
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    c = load_config(path)
    init = particle_init_data(c, 2)
    tune = tmp_path / "logs" / cfg["name"] / "finetune"
    tune.mkdir(parents=True)
    torch.save({"init_x": torch.tensor(init.pos).float(), "init_v": torch.tensor([[0.0, -0.5, 0.0]]).repeat(init.pos.shape[0], 1)}, tune / "init.pt")
    to_render = CD.map_from_alignment(init.size, init.center)
    assert to_render[0][0] != to_render[0][2] and to_render[1] != (0.0, 0.0, 0.0)
    common = ["-c", str(path), "-es", "2", "-dv", "r_0", "--result_root", str(tmp_path / "results")]
    capsys.readouterr()
    render_main(common + ["-vn", "plain"])
    assert "colliders: 2 (not drawn in renders)" in capsys.readouterr().out
    render_main(common + ["-vn", "drawn", "--draw_colliders"])
    assert "colliders: 2 (drawn in renders)" in capsys.readouterr().out
    c.video_data.data.used_views = ["r_0"]
    ds = CameraDataset(c.video_data)
    cam = ds.getCameras("r_0", ds.steps[0])
    root = tmp_path / "results" / cfg["name"]
    names = sorted(p.name for p in (root / "images_drawn").glob("*.png"))
    assert len(names) == 3 and names == sorted(p.name for p in (root / "images_plain").glob("*.png"))
    hit = _hit_of_frame(cam, nodes, 0.0, 0, to_render)
    assert (hit == 0).sum() > 200 and (hit < 0).sum() > 200
    for i, name in enumerate(names):
        a, b = _png(root / "images_plain" / name), _png(root / "images_drawn" / name)
        assert np.abs(a - b)[hit < 0].max() <= (0 if i == 0 else 1)
        # every hit pixel changed, but for those the body in front of the collider covers (not the white background undrawn)
        assert (a != b).any(-1)[hit >= 0].mean() > 0.8 and ((a != b) | (a < 255)).any(-1)[hit >= 0].all()
