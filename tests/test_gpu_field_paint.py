"""GPU: the field paint (csrc/nm_paint.hip through neuma_amd/field_paint.py) against its fp64 definition
(neuma_amd/extras/field_paint.py) on the shared cases of tests/field_paint_cases.py, through the rasterizer, and through the two
drivers' --color_by.  Bounds: field_paint_cases.BOUNDS (four times what the host half of the same code measures on the CPU)."""
import numpy as np
import pytest
import torch

import field_paint_cases as fc
from gpu_util import abs_max, dev, measured, parity, rel_max
from neuma_amd import field_paint as fp
from neuma_amd.extras import field_paint as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return fc.particles()


@pytest.fixture(scope="module")
def ref(P):
    return {q: X.particle_field(q, **{k: P[k] for k in X.NEEDS[q]}) for q in X.QUANTITIES}


@pytest.fixture(scope="module")
def csr_ref():
    """(Bindings on the GPU, q on the GPU, g64 on the CPU): the CSR case and its fp64 values, once"""
    b = fc.csr_bindings(dev())
    q = fc.csr()["q"]
    return b, q.to(dev()), X.gaussian_values(q, b.rowptr.cpu(), b.col.cpu(), b.val.cpu())


# ---------------------------------------------------------------------------------------------------------------- quantities

@pytest.mark.parametrize("quantity", X.QUANTITIES)
def test_quantity_against_fp64(P, ref, quantity):
    d = dev()
    got = fp.particle_field(quantity, **{k: P[k].to(d) for k in X.NEEDS[quantity]}).cpu()
    want = ref[quantity]
    fin = torch.isfinite(want)
    assert got.shape == (fc.N,) and got.dtype == torch.float32
    assert torch.equal(torch.isfinite(got), fin)                                 # no data at the same rows
    assert int((~fin).sum()) >= 8
    parity("field_paint", quantity, rel_max(got[fin], want[fin]), fc.BOUNDS[quantity])
    if quantity == "strain":
        a, b = fc.BLOCKS["identity"]
        parity("field_paint", "strain of the identity block (abs)", float(got[a:b].abs().max()), fc.STRAIN_IDENTITY_ABS)
    if quantity == "volume":
        a, b = fc.BLOCKS["identity"]
        assert bool((got[a:b] == 1.0).all())


def test_unread_arrays_are_not_needed_and_read_ones_are(P):
    d = dev()
    from neuma_amd import NeumaHipError, _lib as L
    q = torch.empty(8, dtype=torch.float32, device=d)
    F = P["F"][:8].to(d).contiguous()
    with pytest.raises(NeumaHipError, match="pressure reads stress"):
        L.check(L.lib().nm_particle_field(8, 4, None, None, L.ptr(F), None, None, L.ptr(q), L.stream_ptr(d)), "nm_particle_field")
    # every other array NULL
    L.check(L.lib().nm_particle_field(8, 3, None, None, L.ptr(F), None, None, L.ptr(q), L.stream_ptr(d)), "nm_particle_field")
    assert torch.equal(q, fp.particle_field("strain", F=F))
    assert fp.particle_field("speed", v=torch.empty(0, 3, device=d)).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- paint

def test_paint_against_fp64(csr_ref):
    b, q, g64 = csr_ref
    c = fc.csr()
    nodata = torch.tensor(sorted(c["empty"] + c["zero_weight"] + c["touching"]))
    fin = torch.isfinite(g64)
    assert torch.equal(torch.nonzero(~fin).reshape(-1), nodata)
    for name, rng in (("rainbow", (-1.0, 6.5)), ("heat", None), ("coolwarm", (0.0, 2.0))):
        shs, g = fp.paint(q, b, name, rng)
        assert shs.shape == (fc.K_CSR, 1, 3) and g.shape == (fc.K_CSR,) and shs.dtype == g.dtype == torch.float32
        g, shs = g.cpu(), shs.cpu()
        assert torch.equal(torch.isfinite(g), fin)
        parity("field_paint", f"g ({name})", rel_max(g[fin], g64[fin]), fc.G_BOUND)
        used = rng if rng is not None else (float(g[fin].min()), float(g[fin].max()))
        if rng is None:                                                          # the device's range is the fp32 g's own, exactly
            assert used == X.data_range(g.double())
        want = X.colors(g64, used if rng is not None else X.data_range(g64), name)
        rgb = shs[:, 0].double() * X.C0 + 0.5
        err = abs_max(rgb, want)
        # (here the error of g passes through the map's slope, up to n - 1 per unit t, so the map case's bound does not apply)
        bound = fc.CSR_COLOR_ABS
        assert bound < 1.0 / 1020.0
        parity("field_paint", f"colour ({name}, abs)", err, bound)
        assert float(shs[nodata].abs().max()) == 0.0                             # exactly the no-data colour: (0.5 - 0.5) / C0
        assert float(shs[fin].abs().max()) > 0.5


def test_direct_path_and_device_range_give_the_same_bits(csr_ref):
    b, q, _ = csr_ref
    d = dev()
    _, g = fp.paint_raw(q, b, want_dc=False)
    r_dev = fp.field_range(g)
    lo, hi = (float(a) for a in r_dev.cpu())
    r_host = torch.tensor([lo, hi], dtype=torch.float32, device=d)
    for name in ("heat", "coolwarm"):
        dc_csr, g_csr = fp.paint_raw(q, b, name, r_dev)                         # one launch: row walk and colour
        dc_dir, g_dir = fp.paint_raw(g, None, name, r_dev)                       # rowptr == NULL on the values themselves
        dc_host, _ = fp.paint_raw(q, b, name, r_host)
        assert torch.equal(g_csr.view(torch.int32), g.view(torch.int32)) and torch.equal(g_dir.view(torch.int32), g.view(torch.int32))
        assert torch.equal(dc_csr.view(torch.int32), dc_dir.view(torch.int32))
        assert torch.equal(dc_csr.view(torch.int32), dc_host.view(torch.int32))
    shs, g2 = fp.paint(q, b, "heat")                                              # the public two-call form
    assert torch.equal(shs[:, 0].view(torch.int32), fp.paint_raw(q, b, "heat", r_dev)[0].view(torch.int32))
    # g_out alone, dc_out alone
    dc_only, none = fp.paint_raw(q, b, "heat", r_dev, want_g=False)
    assert none is None and torch.equal(dc_only.view(torch.int32), shs[:, 0].contiguous().view(torch.int32))


@pytest.mark.parametrize("name", sorted(X.COLORMAPS))
def test_colours_on_between_and_outside_the_knots(name):
    c = fc.color_case()
    shs, g = fp.paint(c["g"].to(dev()), None, name, (c["lo"], c["hi"]))
    assert torch.equal(g.cpu(), c["g"])
    rgb = shs[:, 0].cpu().double() * X.C0 + 0.5
    want = X.colors(c["g"], (c["lo"], c["hi"]), name)
    parity("field_paint", f"map {name} (abs)", abs_max(rgb, want), fc.COLOR_ABS)
    assert measured(float((rgb[c["outside"]] - want[c["outside"]]).abs().max()), "clamped ends") <= 1e-7


# ---------------------------------------------------------------------------------------------------------------- range

@pytest.mark.parametrize("K", [1, 255, 257, 70000])
def test_range_is_exact(K):
    d = dev()
    g = torch.Generator().manual_seed(K)
    v = (100.0 * torch.randn(K, generator=g)).to(d)
    if K > 1:
        v[::7] = float("nan")
        v[3::11] = float("inf")
        v[5::13] = float("-inf")
        v[K - 1] = -1234.5                                                       # the extremes in the last (partial) wave / block
        v[K - 2] = 4321.0
    fin = v[torch.isfinite(v)]
    r = fp.field_range(v)
    want = torch.stack([fin.min(), fin.max()]) if K > 1 else torch.stack([fin.min(), fin.min() + 1.0])      # (one value: widened)
    assert torch.equal(r, want)
    assert torch.equal(fp.field_range(v, fp.empty_range(d), fold=True), torch.stack([fin.min(), fin.max()]))
    assert torch.equal(fp.field_range(v), r)


def test_running_range_over_three_frames_and_the_widening_rule():
    d = dev()
    g = torch.Generator().manual_seed(9)
    frames = [(s * torch.randn(5000, generator=g) + o).to(d) for s, o in ((1.0, 0.0), (3.0, 2.0), (0.5, -1.0))]
    frames[1][::3] = float("nan")
    run = fp.empty_range(d)
    for f in frames:
        fp.field_range(f, run, fold=True)
    allv = torch.cat(frames)
    allv = allv[torch.isfinite(allv)]
    assert torch.equal(run, torch.stack([allv.min(), allv.max()]))
    # a frame without data leaves the pair alone; an empty pair stays empty
    fp.field_range(torch.full((300,), float("nan"), device=d), run, fold=True)
    assert torch.equal(run, torch.stack([allv.min(), allv.max()]))
    assert torch.equal(fp.field_range(torch.full((300,), float("inf"), device=d), fp.empty_range(d), fold=True).cpu(),
                       torch.tensor([float("inf"), float("-inf")]))
    # mode 0: no finite value -> [0, 1]; a constant -> [c, c + 1]; no value at all -> [0, 1]
    assert fp.field_range(torch.tensor([float("nan"), float("inf"), float("-inf")] * 100, device=d)).tolist() == [0.0, 1.0]
    assert fp.field_range(torch.full((1000,), 2.5, device=d)).tolist() == [2.5, 3.5]
    assert fp.field_range(torch.tensor([7.0, float("nan")], device=d)).tolist() == [7.0, 8.0]
    assert fp.field_range(torch.empty(0, device=d)).tolist() == [0.0, 1.0]
    # ... and such a frame is painted: a constant field sits at t = 0, a field without data in the no-data colour
    shs, _ = fp.paint(torch.full((10,), 2.5, device=d), None, "heat")
    assert float((shs * X.C0 + 0.5).abs().max()) == 0.0
    shs, _ = fp.paint(torch.full((10,), float("nan"), device=d), None, "heat")
    assert float(shs.abs().max()) == 0.0


def test_painter_frames_share_one_range_over_objects(P, csr_ref):
    """Two objects with their own bindings: the values are those of per-object paints, the range is shared, the running range is the
    overall one, and nothing of it needs the host before overall_range()."""
    d = dev()
    b, q, _ = csr_ref
    n = fc.N_CSR
    v = torch.zeros(2 * n, 3, device=d)
    v[:n, 0] = q.nan_to_num(0.0, 0.0, 0.0).abs()
    v[n:, 1] = 3.0 * q.nan_to_num(0.0, 0.0, 0.0).abs() + 1.0
    auto = fp.FieldPainter("speed")
    shs = auto.frame(None, v, None, None, [b, b], sections=[n, n])
    assert shs.shape == (2 * fc.K_CSR, 1, 3) and auto.last_q.shape == (2 * n,)
    g = auto.last_g
    _, g0 = fp.paint_raw(auto.last_q[:n], b, want_dc=False)
    _, g1 = fp.paint_raw(auto.last_q[n:], b, want_dc=False)
    assert torch.equal(g.view(torch.int32), torch.cat([g0, g1]).view(torch.int32))
    fin = g[torch.isfinite(g)]
    want, _ = fp.paint_raw(g, None, "heat", torch.stack([fin.min(), fin.max()]), want_g=False)
    assert torch.equal(shs[:, 0].contiguous().view(torch.int32), want.view(torch.int32))
    shs2 = auto.frame(None, 2.0 * v, None, None, [b, b], sections=[n, n])
    assert torch.equal(shs2.view(torch.int32), shs.view(torch.int32))            # its own range: the same picture at twice the speed
    assert auto.overall_range() == (float(fin.min()), 2.0 * float(fin.max()))
    fixed = fp.FieldPainter("speed", "heat", (float(fin.min()), float(fin.max())))
    assert torch.equal(fixed.frame(None, v, None, None, [b, b], sections=[n, n]).view(torch.int32), shs.view(torch.int32))
    assert fixed.running is None
    # a quantity that reads the stress asks stress_fn for it, once, with the frame's own F
    calls = []
    F, tau = P["F"][:n].to(d), P["stress"][:n].to(d)

    def stress_fn(Fin):
        calls.append(Fin)
        return tau
    vm = fp.FieldPainter("von_mises")
    vm.frame(None, None, F, stress_fn, b)
    assert len(calls) == 1 and calls[0] is F
    assert torch.equal(vm.last_q, fp.particle_field("von_mises", F=F, stress=tau))
    dsp = fp.FieldPainter("displacement")
    x = P["x"][:n].to(d)
    dsp.frame(x, None, None, None, b)
    assert float(dsp.last_q.abs().max()) == 0.0                                  # measured from the first frame's positions
    dsp.frame(x + 0.25, None, None, None, b)
    assert abs(float(dsp.last_q[0]) - 0.25 * 3 ** 0.5) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- rasterizer

@torch.no_grad()
def test_painted_gaussians_render_as_their_colour():
    from neuma_amd import synth
    from neuma_amd.tune import diff_rasterization
    d = dev()
    K = 300
    g = torch.Generator().manual_seed(4)
    xyz = (0.5 + 0.15 * torch.randn(K, 3, generator=g)).to(d)
    s = 0.02 + 0.02 * torch.rand(K, 3, generator=g)
    cov = torch.zeros(K, 6)
    cov[:, 0], cov[:, 3], cov[:, 5] = s[:, 0] ** 2, s[:, 1] ** 2, s[:, 2] ** 2
    cov, opa = cov.to(d), (0.3 + 0.6 * torch.rand(K, 1, generator=g)).to(d)
    cam = synth.ring_cameras(1, 64, 48, device=d)[0]
    bg = torch.zeros(3, device=d)
    # 0.75 over [0, 1] through `rainbow` (5 knots): t (n - 1) = 3 exactly, the knot (1, 1, 0), with no rounding on the way
    shs, _ = fp.paint(torch.full((K,), 0.75, device=d), None, "rainbow", (0.0, 1.0))
    host = ((torch.tensor([1.0, 1.0, 0.0]) - 0.5) / torch.tensor(X.C0, dtype=torch.float32)).to(d).expand(K, 1, 3).contiguous()
    assert torch.equal(shs, host)
    a = diff_rasterization(xyz, None, None, cam, bg, 0, cov, opa, shs)
    b = diff_rasterization(xyz, None, None, cam, bg, 0, cov, opa, host)
    assert torch.equal(a, b)
    cover = a[0] > 0.05
    assert int(cover.sum()) > 200
    assert float((a[0] - a[1]).abs().max()) == 0.0 and float(a[2].abs().max()) < 1e-6      # yellow wherever anything shows
    # a Gaussian alone shows exactly rgb where it saturates: alpha-weighted, so red / green equal the accumulated alpha
    alpha = diff_rasterization(xyz, None, None, cam, bg, 0, cov, opa, shs, force_mask_data=True)
    assert measured(float((a[0] - alpha[0]).abs().max()), "painted colour vs accumulated alpha") < 2e-6


# ---------------------------------------------------------------------------------------------------------------- entry points

def _png_bytes(folder):
    return {p.name: p.read_bytes() for p in sorted(folder.glob("*.png"))}


def test_render_color_by_adds_a_sequence_and_moves_nothing(tmp_path, capsys):
    """The ordinary frames of a run with --color_by are those of the same command without it.  Byte for byte wherever two runs can
    be compared at all: the simulator's scatters use float atomics, and two runs of this very command WITHOUT the flag already differ
    in the last bits of F from the first step on (measured, five runs, every pair: |dF| 5e-11 after step 1, 1e-7 after step 2, up to
    9e-7 after step 3; x still bitwise equal after step 3, different after step 4; one run of six differed by one 8-bit level in two
    frames).  So:
      - frame 0 (the un-deformed kernels, no simulator behind it) is compared between the two commands, byte for byte;
      - every frame the run with the flag wrote is compared, byte for byte, with what the driver's ordinary path renders from the
        state that run handed to on_frame: with the simulator's noise taken out, the flag moves no byte;
      - between the two commands the positions agree to the noise two runs without the flag show (2e-6), the frames to one 8-bit level."""
    from PIL import Image
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import evaluate as ev
    from neuma_amd.finetune import main as finetune_main
    import yaml
    path, _ = _write_experiment(tmp_path, frames=2)                               # (velocity.num_frames is 2)
    short = yaml.safe_load(path.read_text())                                     # (the roll-out needs an experiment: the shortest one)
    short["constitution"]["num_epochs"] = short["velocity"]["num_epochs"] = 1
    path.write_text(yaml.safe_dump(short, sort_keys=False))
    finetune_main(["-c", str(path)])
    capsys.readouterr()
    common = ["-c", str(path), "-es", "3", "-dt", "0.004", "-dv", "r_0", "-vn", "plain"]

    def config(extra):
        args = ev.parse_args(common + extra)
        cfg = ev.load_config(args.config)
        cfg.update({k: val for k, val in vars(args).items() if k != "config"})          # (what ev.main does)
        return cfg

    def run(extra):
        """ev.main(argv) with a hook on the frames: step -> what the frame was rendered from"""
        seen = {}
        ev.evaluate(config(extra), on_frame=lambda step, fr: seen.__setitem__(step, {k: fr[k].detach().clone() for k in ("x", "F", "means3D", "deform_grad")}))
        return seen, capsys.readouterr().out.splitlines()

    flag = ["--result_root", str(tmp_path / "painted"), "--color_by", "speed", "--color_range", "0", "1"]
    seen_a, plain_lines = run(["--result_root", str(tmp_path / "plain")])
    seen_b, painted_lines = run(flag)
    a, b = tmp_path / "plain" / "tinyball-v1", tmp_path / "painted" / "tinyball-v1"
    plain, same = _png_bytes(a / "images_plain"), _png_bytes(b / "images_plain")
    assert sorted(plain) == sorted(same) == [f"r_0_{i:03d}.png" for i in range(4)]
    assert plain["r_0_000.png"] == same["r_0_000.png"]                           # byte for byte
    # the ordinary path of the driver, by hand, on the states of the run with the flag
    cfg = config(flag)
    cfg.video_data.data.init_frame = cfg.get("init_frame")
    cfg.video_data.data.used_views = ["r_0"]
    env = ev.setup(cfg, dev(), for_eval=True)
    capsys.readouterr()
    gaussians, cam = env["gaussians"], env["dataset"].getCameras("r_0", env["dataset"].steps[0])
    white = torch.ones(3, device=dev())
    for k in sorted(seen_b):
        img = ev.diff_rasterization(seen_b[k]["means3D"], seen_b[k]["deform_grad"], gaussians, cam, white, scaling_modifier=1.0)
        ev.save_image(img, tmp_path / "by_hand.png")
        assert (tmp_path / "by_hand.png").read_bytes() == same[f"r_0_{k:03d}.png"], k      # byte for byte
    for k in sorted(seen_a):
        for key in ("x", "means3D"):         # (the bound tests/test_gpu_entrypoints.py holds two runs of one scene to, there after 12 steps)
            assert measured(float((seen_a[k][key] - seen_b[k][key]).abs().max()), f"{key} after step {k}: with vs without --color_by (abs)") < 2e-6
        print(f"step {k}: |dF| between the two runs {float((seen_a[k]['F'] - seen_b[k]['F']).abs().max()):.2e}")      # (a few ulps of 1, growing)
        lv = np.abs(np.array(Image.open(a / "images_plain" / f"r_0_{k:03d}.png")).astype(np.int32)
                    - np.array(Image.open(b / "images_plain" / f"r_0_{k:03d}.png")).astype(np.int32)).max()
        assert measured(lv, f"frame {k}: 8-bit levels, with vs without --color_by") <= 1
    speed = _png_bytes(b / "images_plain_speed")
    assert sorted(speed) == sorted(plain)
    assert not (a / "images_plain_speed").exists() and sorted(p.name for p in a.iterdir()) == ["images_plain"]
    assert not any(l.startswith("color_by") or "overall range" in l for l in plain_lines)      # (tmp_path itself holds the word)
    said = [l for l in painted_lines if l.startswith("color_by")]
    assert said == ["color_by speed (heat): range 0 .. 1"]                       # an explicit range: nothing to report at the end
    assert len(painted_lines) == len(plain_lines) + 1
    # the painted frames show the heat map of the falling body on white: red / yellow pixels, no blue ones
    last = np.array(Image.open(b / "images_plain_speed" / "r_0_003.png")).astype(np.int32)
    body = (last < 250).any(axis=2)
    assert int(body.sum()) > 50 and bool((last[body][:, 0] >= last[body][:, 2]).all())
    first = np.array(Image.open(b / "images_plain_speed" / "r_0_000.png")).astype(np.int32)
    assert np.abs(first - last).max() > 5                                        # the speed changed under gravity


def test_inference_color_by_von_mises_exports_gaussians_and_particle_values(tmp_path, capsys):
    import yaml
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import io as nio, synth
    from neuma_amd.inference import main as inference_main
    from neuma_amd.replay import main as replay_main
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))}, raw / "plasticine_0300.pt")
    import shutil
    shutil.copytree(assets / "tinyball", assets / "tinycat")
    for f in (assets / "tinycat").glob("particles.npz"):
        f.unlink()

    def obj(name, ckpt, lo):
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=dict(sh_degree=3),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 0.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"], views=["r_0"]))

    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=32, eps=6e-7),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45), obj("tinycat", "plasticine_0300.pt", 0.02)])
    demo = tmp_path / "multiobj-tiny.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    steps = 3
    seen = {}
    capsys.readouterr()
    import neuma_amd.inference as inf
    args = inf.parse_args(["-c", str(demo), "-s", str(steps), "-vn", "pair", "-dv", "r_0", "--color_by", "von_mises", "--save_gaussians", "g",
                           "--save_particles", "p", "--result_root", str(tmp_path / "results")])
    c = inf.load_config(args.config)
    c.update({k: val for k, val in vars(args).items() if k != "config"})          # (main() itself, with a hook on the frames)
    inf.inference(c, on_frame=lambda step, fr: seen.__setitem__(step, (fr["x"].clone(), fr["F"].clone(), fr["values"].clone())))
    lines = capsys.readouterr().out.splitlines()
    res = tmp_path / "results" / "inference"
    names = [f"{i:03d}.ply" for i in range(steps + 1)]
    assert sorted(p.name for p in (res / "gaussians_g").glob("*.ply")) == names
    assert sorted(p.name for p in (res / "gaussians_g_von_mises").glob("*.ply")) == names
    assert sorted(p.name for p in (res / "images_pair_von_mises").glob("*.png")) == sorted(p.name for p in (res / "images_pair").glob("*.png"))
    assert len(list((res / "images_pair").glob("*.png"))) == steps + 1
    # the painted files: the frame's Gaussians, degree 0, the painted colour
    full, flat = nio.read_ply_vertices(res / "gaussians_g" / "003.ply"), nio.read_ply_vertices(res / "gaussians_g_von_mises" / "003.ply")
    assert list(flat) == nio.gaussian_attribute_names(3, 0)
    for k in ("x", "y", "z", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"):
        assert np.array_equal(np.asarray(full[k]).view(np.uint32), np.asarray(flat[k]).view(np.uint32)), k
    rgb = np.stack([flat[f"f_dc_{i}"] for i in range(3)], 1) * X.C0 + 0.5
    assert rgb.min() > -1e-6 and rgb.max() < 1 + 1e-6 and rgb.std() > 0.01                # colours of a map, and not one colour
    # ... and replay shows them from the dataset's camera
    assert replay_main(["-s", str(res / "gaussians_g_von_mises"), "-c", str(demo), "-dv", "r_0", "--sh_degree", "0", "-o", str(tmp_path / "replay")]) == 0
    assert len(list((tmp_path / "replay").glob("r_0_*.png"))) == steps + 1
    # the particle files carry the quantity: the values of the frame's own state
    E = None
    for step in range(1, steps + 1):
        v = nio.read_ply_vertices(res.parent / "inference_states" / "states_p" / f"{step:03d}.ply")
        assert list(v) == ["x", "y", "z", "von_mises"]
        x, F, vals = seen[step]
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), x.cpu().numpy())
        assert np.array_equal(np.asarray(v["von_mises"]).view(np.uint32), vals.cpu().numpy().view(np.uint32))
        fin = np.isfinite(v["von_mises"])
        assert fin.mean() > 0.99 and float(v["von_mises"][fin].max()) > 0
    # values = particle_field of the frame's state: the stress is E(F) of the frame's own F, per object
    from neuma_amd.inference import load_object
    from neuma_amd.material import ComposeMaterial
    objects = [load_object(o, assets, steps, dev()) for o in inf.load_config(str(demo)).objects]
    secs = [o.init_data.num_particles for o in objects]
    E = ComposeMaterial([o.elasticity for o in objects], secs).to(dev()).eval()
    x, F, vals = seen[steps]
    with torch.no_grad():
        want = fp.particle_field("von_mises", F=F, stress=E(F))
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(vals), fin) and torch.equal(vals[fin], want[fin])
    x0, F0, vals0 = seen[0]                                                      # frame 0: F = I and the stress of I
    assert float((F0 - torch.eye(3, device=F0.device)).abs().max()) == 0.0
    with torch.no_grad():
        assert torch.equal(vals0, fp.particle_field("von_mises", F=F0, stress=E(F0)))
    # the range: said once at the start, reported once at the end with the flag to pass
    assert sum("every frame is scaled by its own range" in l for l in lines) == 1
    overall = [l for l in lines if l.startswith("color_by von_mises: overall range")]
    assert len(overall) == 1 and "--color_range " in overall[0]
    lo, hi = (float(t) for t in overall[0].split("--color_range ")[1].split()[:2])
    assert hi > lo >= 0.0
