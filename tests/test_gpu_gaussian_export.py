"""GPU: nm_gaussian_deform and the export of roll-out frames as 3DGS .ply files (neuma_amd/export.py, `render --save_gaussians`,
`inference --save_gaussians`, `python -m neuma_amd.replay`).

1 kernel against fp64 on the families of gaussian_export_cases.py: per family the largest over kept rows of
  max|nm_gaussian_activate(outputs) - Sigma'_64| / max|Sigma'_64| is at most max(4 x yardstick, 2e-6); the yardstick is the same
  error of the same computation by code older than the kernel (F @ L in torch fp32 on the device, nm_svd3_fwd, log|s|, exp, square,
  U diag U^T).  The families `zero` and `scaled_out` are dropped from the comparison (gaussian_export_cases.py says why); on ALL rows
  of ALL families the outputs are finite, | |q| - 1 | <= 1e-6 and r >= 0.
2 shapes: K = 1, 257 (block tail), 1000; F = NULL is the explicit identity bit for bit; scale_modifier; overlapping buffers refused.
3 the Python layer.
4 what the feature is for: a frame written by `evaluate(save_gaussians=...)` and rendered again by replay.render_sequence is the image
  the roll-out produced, to max(4 x yardstick, 1e-6) per pixel, the yardstick being the image of the existing-code covariance of 1.
5 the entry points."""
import math

import numpy as np
import pytest
import torch
import yaml

import gaussian_export_cases as gc
from gpu_util import dev, measured, parity

pytestmark = pytest.mark.gpu

PIXEL_FLOOR = 1e-6


def _svd(M):
    from neuma_amd.svd import SVDFunction
    return SVDFunction.apply(M)


def _cov6_of(ls, rot):
    from neuma_amd.render import gaussian_activate
    return gaussian_activate(ls, rot, None, 1.0, want_opacity=False)[0]


def _quats_ok(ls_out, q):
    assert bool(torch.isfinite(ls_out).all()) and bool(torch.isfinite(q).all())
    assert float((q.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert bool((q[:, 0] >= 0).all())


@pytest.fixture(scope="module")
def cases():
    return gc.inputs(0)


# ------------------------------------------------------------------ 1: the kernel against fp64

@pytest.mark.parametrize("name", list(gc.inputs(0)))
def test_kernel_family_within_existing_code_noise(cases, name):
    from neuma_amd.export import gaussian_deform
    F, ls, rot = (t.to(dev()) for t in cases[name])
    assert F.shape[0] <= 1000
    lo, q = gaussian_deform(ls, rot, F)
    _quats_ok(lo, q)
    if name in gc.DROPPED:
        return
    S = gc.sigma64(*cases[name])
    keep = gc.kept(S)
    assert keep.mean() >= gc.KEEP_SHARE
    err = gc.family_error(gc.full_from_cov6(_cov6_of(lo, q).cpu().numpy()), S, keep)
    yard = gc.family_error(gc.yardstick_cov(F, ls, rot, _svd).double().cpu().numpy(), S, keep)
    # (both figures go to the parity log: `measured`, and the yardstick as the record's reference_fp32_vs_fp64)
    parity("gaussian_deform", f"{name}: max|activate(outputs) - cov64| / max|cov64|", err, max(gc.MARGIN * yard, gc.FLOOR), noise=yard)


# ------------------------------------------------------------------ 2: shapes

@pytest.mark.parametrize("K", [1, 257, 1000])
def test_shapes_identity_and_modifier(cases, K):
    from neuma_amd.export import gaussian_deform
    F, ls, rot = (t[:K].contiguous().to(dev()) for t in cases["cond1e3"])
    full = gaussian_deform(*(t.to(dev()) for t in (cases["cond1e3"][1], cases["cond1e3"][2], cases["cond1e3"][0])))
    lo, q = gaussian_deform(ls, rot, F)
    assert lo.shape == (K, 3) and q.shape == (K, 4)
    assert torch.equal(lo, full[0][:K]) and torch.equal(q, full[1][:K]), "a Gaussian's result depends on its block-mates"
    # F = NULL is the explicit identity, bit for bit
    a = gaussian_deform(ls, rot, None)
    b = gaussian_deform(ls, rot, torch.eye(3, device=dev()).expand(K, 3, 3).contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # scale_modifier 0.5 is log_scales + log 0.5, within the bound of the family comparison
    Fc, lc, rc = (t[:K] for t in cases["cond1e3"])
    S = gc.sigma64(Fc, lc, rc, 0.5)
    keep = gc.kept(S)
    half = gaussian_deform(ls, rot, F, 0.5)
    _quats_ok(*half)
    err = gc.family_error(gc.full_from_cov6(_cov6_of(*half).cpu().numpy()), S, keep)
    yard = gc.family_error(gc.yardstick_cov(F, ls, rot, _svd, 0.5).double().cpu().numpy(), S, keep)
    parity("gaussian_deform", f"K={K} modifier 0.5 against the definition", err, max(gc.MARGIN * yard, gc.FLOOR), noise=yard)
    shifted = gaussian_deform((ls + math.log(0.5)).contiguous(), rot, F)
    err = gc.family_error(gc.full_from_cov6(_cov6_of(*shifted).cpu().numpy()), S, keep)
    parity("gaussian_deform", f"K={K} log_scales + log 0.5 against the definition at modifier 0.5", err, max(gc.MARGIN * yard, gc.FLOOR), noise=yard)


def test_overlapping_buffers_and_bad_arguments_are_refused(cases):
    from neuma_amd import _lib as L
    K = 64
    F, ls, rot = (t[:K].contiguous().to(dev()) for t in cases["baseline"])
    lo, q = torch.empty_like(ls), torch.empty_like(rot)
    fn, st = L.lib().nm_gaussian_deform, L.stream_ptr(dev())
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(q), st) == 0
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(ls), L.ptr(q), st) == -1            # in place on the log-scales
    assert b"overlap" in L.lib().nm_last_error()
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(rot), st) == -1           # in place on the quaternions
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(F), st) == -1             # an output inside F
    both = torch.empty(K * 4 + 4, device=dev())
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(both), L.ptr(both[4:]), st) == -1    # the outputs overlap each other
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), q.data_ptr() + 4, st) == -1     # rot_out not 16-byte aligned
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, None, L.ptr(q), st) == -1
    assert fn(-1, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(q), st) == -1
    assert fn(0, None, None, None, 1.0, None, None, st) == 0
    torch.cuda.synchronize()
    ref_lo, ref_q = lo.clone(), q.clone()
    assert fn(K, L.ptr(ls), L.ptr(rot), L.ptr(F), 1.0, L.ptr(lo), L.ptr(q), st) == 0               # and it is deterministic
    assert torch.equal(lo, ref_lo) and torch.equal(q, ref_q)


# ------------------------------------------------------------------ 3: the Python layer

def _model(K, deg, device, seed=2):
    from neuma_amd.render.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    n = (deg + 1) ** 2
    t = [torch.randn(K, 3, generator=g), torch.randn(K, 1, 3, generator=g), torch.randn(K, n - 1, 3, generator=g),
         math.log(1e-2) + torch.randn(K, 3, generator=g), torch.randn(K, 4, generator=g), torch.randn(K, 1, generator=g)]
    return GaussianModel(deg).set_params(*(x.to(device) for x in t))


def test_deformed_gaussians_shares_what_does_not_change():
    from neuma_amd import NeumaHipError
    from neuma_amd.export import deformed_gaussians
    K = 300
    m = _model(K, 1, dev())
    g = torch.Generator().manual_seed(4)
    means = torch.randn(K, 3, generator=g).to(dev())
    F = (torch.eye(3)[None] + 0.3 * torch.randn(K, 3, 3, generator=g)).to(dev())
    out = deformed_gaussians(m, means, F, scaling_modifier=0.7)
    assert out._opacity is m._opacity and out._features_dc is m._features_dc and out._features_rest is m._features_rest
    assert out._xyz.data_ptr() == means.data_ptr() and out.active_sh_degree == 1 and out.get_xyz.device == means.device
    S = gc.sigma64(F.cpu(), m._scaling.cpu(), m._rotation.cpu(), 0.7)
    err = gc.family_error(gc.full_from_cov6(out.get_covariance(1.0).cpu().numpy()), S, np.ones(K, dtype=bool))
    assert measured(err, "deformed_gaussians: get_covariance(1) against F cov F^T at modifier 0.7 (rel)") <= 1e-5
    assert torch.equal(deformed_gaussians(m, means, F.reshape(K, 9), scaling_modifier=0.7)._scaling, out._scaling)
    shs = torch.randn(K, 4, 3, generator=g).to(dev())
    with_shs = deformed_gaussians(m, means, F, shs)
    assert torch.equal(with_shs._features_rest, shs[:, 1:]) and with_shs._features_dc is m._features_dc
    assert torch.equal(with_shs.get_features[:, 1:], shs[:, 1:])
    rest = deformed_gaussians(m, m.get_xyz)                                        # no deformation: the rest covariance
    assert float((rest.get_covariance(1.0) - m.get_covariance(1.0)).abs().max() / m.get_covariance(1.0).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        deformed_gaussians(m, means, F, shs[:, :3])
    bad = F.clone(); bad[7, 1, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        deformed_gaussians(m, means, bad)
    with pytest.raises((NeumaHipError, ValueError)):
        deformed_gaussians(_model(K, 1, "cpu"), means.cpu(), F.cpu())
    with pytest.raises((NeumaHipError, ValueError)):
        deformed_gaussians(m, means.cpu(), F)


# ------------------------------------------------------------------ 4, 5: frames on disk

@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """the tiny experiment of tests/test_gpu_entrypoints.py (3 frames) with stage A's init.pt, written once for this module"""
    from test_gpu_entrypoints import _write_experiment
    from test_gpu_sh_deform import _write_init
    root = tmp_path_factory.mktemp("export_exp")
    path, _ = _write_experiment(root, frames=3)
    _write_init(root, path)
    return root, path


def _with_degree(root, path, deg):
    """the experiment with its kernels cut to SH degree `deg` (own asset folder)"""
    from neuma_amd import io as nio
    from neuma_amd.render.gaussian_model import GaussianModel
    raw = root / "raw"
    full = nio.load_gaussians_ply(raw / "point_cloud.ply", 3)
    g = GaussianModel(deg)
    g.set_params(full._xyz, full._features_dc, full._features_rest[:, :(deg + 1) ** 2 - 1].contiguous(), full._scaling, full._rotation,
                 full._opacity)
    nio.save_gaussians_ply(g, raw / f"point_cloud_sh{deg}.ply")
    cfg = yaml.safe_load(path.read_text())
    cfg["gaussian"].update(sh_degree=deg, kernels_path=str(raw / f"point_cloud_sh{deg}.ply"))
    cfg["sim_data_name"] = f"tinyball{deg}"
    out = root / f"finetune-tiny-sh{deg}.yaml"
    out.write_text(yaml.safe_dump(cfg, sort_keys=False))
    return out


def _pixel_rule(direct, replayed, yard_img, what):
    err = float((replayed - direct).abs().max())
    yard = float((yard_img - direct).abs().max())
    parity("gaussian_export", f"{what}: replayed file against the direct image (max abs pixel)", err, max(gc.MARGIN * yard, PIXEL_FLOOR),
           noise=yard)


@pytest.mark.parametrize("deg,rotate", [(0, False), (1, True)])
def test_replayed_frames_are_the_rollouts_images(experiment, deg, rotate):
    from test_gpu_sh_deform import _eval_cfg
    from neuma_amd import io as nio
    from neuma_amd.config import load_config
    from neuma_amd.evaluate import evaluate
    from neuma_amd.finetune import setup
    from neuma_amd.render import flush_pending
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    from neuma_amd.replay import render_sequence, sequence_paths
    from neuma_amd.tune import diff_rasterization
    root, path = experiment
    pdeg = _with_degree(root, path, deg)
    name, scal = f"rt{deg}", 0.8
    cfg = _eval_cfg(pdeg, root, name, scaling_modifier=scal, **({"rotate_sh": True} if rotate else {}))
    cfg["save_gaussians"] = name
    frames = []
    evaluate(cfg, on_frame=lambda step, f: frames.append(dict(means3D=f["means3D"].clone(), deform_grad=f["deform_grad"].clone(),
                                                              image=f["images"]["r_0"].clone())))
    assert len(frames) == 3
    paths = sequence_paths(root / "results" / cfg.name / f"gaussians_{name}")
    assert [p.name for p in paths] == [f"{i:03d}.ply" for i in range(4)]
    env = setup(load_config(pdeg), dev(), for_eval=True)
    gm, ds = env["gaussians"], env["dataset"]
    cam = ds.getCameras("r_0", ds.steps[0])
    white = torch.ones(3, device=dev())
    K = gm.get_xyz.shape[0]
    with torch.no_grad():
        first = nio.load_gaussians_ply(paths[0], deg, device=dev())
        assert first.get_xyz.shape[0] == K and torch.equal(first._features_rest, gm._features_rest) and torch.equal(first._xyz, gm._xyz)
        for f, (no, imgs) in zip(frames, render_sequence(paths[1:], [cam], white, deg)):
            flush_pending()
            F = f["deform_grad"].reshape(-1, 3, 3)
            shs = rotate_shs_by_deformation(gm.get_features, F) if rotate else gm.get_features
            saved = nio.load_gaussians_ply(paths[no], deg, device=dev())
            assert torch.equal(saved._xyz, f["means3D"]) and torch.equal(saved._opacity, gm._opacity)
            assert torch.equal(saved.get_features, shs), "f_dc / f_rest are not the coefficients the frame was rendered with"
            if rotate:
                assert not torch.equal(saved._features_rest, gm._features_rest)
            Sy = gc.yardstick_cov(F.contiguous(), gm._scaling.detach(), gm._rotation.detach(), _svd, scal)
            cov_y = torch.stack([Sy[:, 0, 0], Sy[:, 0, 1], Sy[:, 0, 2], Sy[:, 1, 1], Sy[:, 1, 2], Sy[:, 2, 2]], -1).contiguous()
            yard_img = diff_rasterization(f["means3D"], None, None, cam, white, deg, cov_y, gm.get_opacity, shs.contiguous())
            flush_pending()
            _pixel_rule(f["image"], imgs[0], yard_img, f"sh_degree {deg} rotate_sh {rotate} frame {no}")
    moved = float((frames[-1]["image"] - frames[0]["image"]).abs().max())
    assert moved > 1e-3, "the body must move between the frames, or the comparison says nothing"


def _png(path):
    from PIL import Image
    return np.array(Image.open(path)).astype(np.int32)


def test_render_and_replay_entry_points(experiment):
    from neuma_amd.evaluate import main as render_main
    from neuma_amd.replay import main as replay_main
    root, path = experiment
    res = root / "results-ep"
    render_main(["-c", str(path), "-vn", "ep", "-es", "3", "-dv", "r_0", "--save_gaussians", "ep", "--result_root", str(res)])
    out = res / "tinyball-v1"
    gdir = out / "gaussians_ep"
    assert sorted(p.name for p in gdir.glob("*")) == [f"{i:03d}.ply" for i in range(4)]
    assert replay_main(["-s", str(gdir), "-c", str(path), "-dv", "r_0", "-o", str(res / "again")]) in (None, 0)
    assert sorted(p.name for p in (res / "again").glob("*.png")) == [f"r_0_{i:03d}.png" for i in range(4)]
    for i in range(4):
        a, b = _png(out / "images_ep" / f"r_0_{i:03d}.png"), _png(res / "again" / f"r_0_{i:03d}.png")
        assert measured(np.abs(a - b).max(), f"frame {i}: replayed PNG against the direct PNG (8-bit levels)") <= 1
    assert np.abs(_png(res / "again" / "r_0_003.png") - _png(res / "again" / "r_0_000.png")).max() > 5
    # another camera, default output folder; and an export without any view renders nothing
    assert replay_main(["-s", str(gdir), "-c", str(path), "-dv", "r_1"]) in (None, 0)
    assert sorted(p.name for p in (gdir / "replay").glob("*.png")) == [f"r_1_{i:03d}.png" for i in range(4)]
    with pytest.raises(ValueError, match="not in the dataset"):
        replay_main(["-s", str(gdir), "-c", str(path), "-dv", "nowhere"])
    render_main(["-c", str(path), "-vn", "noview", "-es", "1", "--save_gaussians", "noview", "--result_root", str(res)])
    assert sorted(p.name for p in (out / "gaussians_noview").glob("*")) == ["000.ply", "001.ply"]
    assert list((out / "images_noview").glob("*.png")) == []
    # without the option nothing of the kind is written
    render_main(["-c", str(path), "-vn", "plain", "-es", "1", "-dv", "r_0", "--result_root", str(res)])
    assert sorted(p.name for p in out.iterdir() if p.name.endswith("plain")) == ["images_plain"]


def test_inference_entry_point_saves_all_objects_in_one_file(experiment):
    """the two-object scene of tests/test_gpu_entrypoints.py (one box above the other), each object with its own scaling_modifier"""
    import shutil
    from neuma_amd import io as nio, synth
    from neuma_amd.config import load_config
    from neuma_amd.dataset import CameraDataset
    from neuma_amd.infer import simulate_objects
    from neuma_amd.inference import load_object, main as inference_main
    from neuma_amd.render import flush_pending
    from neuma_amd.replay import main as replay_main, render_sequence
    from neuma_amd.sim import MPMModelBuilder
    from neuma_amd.tune import diff_rasterization
    root, path = experiment
    base = yaml.safe_load(path.read_text())
    raw, assets = root / "raw", root / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))}, raw / "plasticine_0300.pt")
    if not (assets / "tinycat").exists():
        shutil.copytree(assets / "tinyball", assets / "tinycat")
        for f in (assets / "tinycat").glob("particles.npz"):
            f.unlink()

    def obj(name, ckpt, lo, scal):
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=dict(sh_degree=3, scaling_modifier=scal),
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 8.0]), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"], views=["r_0"]))

    cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
               video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
               sim=dict(base["sim"], num_grids=32, eps=6e-7),
               objects=[obj("tinyball", "jelly_0300.pt", 0.45, 1.0), obj("tinycat", "plasticine_0300.pt", 0.02, 0.6)])
    demo = root / "multiobj-export.yaml"
    demo.write_text(yaml.safe_dump(cfg, sort_keys=False))
    steps, res = 3, root / "results-inf"
    inference_main(["-c", str(demo), "-s", str(steps), "-vn", "pair", "-dv", "r_0", "--save_gaussians", "pair", "--result_root", str(res)])
    gdir = res / "inference" / "gaussians_pair"
    assert sorted(p.name for p in gdir.glob("*")) == [f"{i:03d}.ply" for i in range(steps + 1)]            # one file per frame
    c = load_config(demo)
    objects = [load_object(o, assets, steps, dev()) for o in c.objects]
    counts = [int(o.gaussians.get_xyz.shape[0]) for o in objects]
    assert [o.scaling for o in objects] == [1.0, 0.6]
    for p in gdir.glob("*.ply"):
        assert nio.load_gaussians_ply(p, 3).get_xyz.shape[0] == sum(counts)
    assert replay_main(["-s", str(gdir), "-c", str(demo), "-dv", "r_0", "--sh_degree", "3"]) in (None, 0)
    for i in range(steps + 1):
        a, b = _png(res / "inference" / "images_pair" / f"r_0_{i:03d}.png"), _png(gdir / "replay" / f"r_0_{i:03d}.png")
        assert measured(np.abs(a - b).max(), f"inference frame {i}: replayed PNG against the direct PNG (8-bit levels)") <= 1
    # ---- the operators by hand, under the rule of the round trip above
    model = MPMModelBuilder().parse_cfg(c.sim).finalize(dev(), False)
    ds = CameraDataset(c.video_data)
    cam = ds.getCameras("r_0", ds.steps[0])
    white = torch.ones(3, device=dev())
    frames = list(simulate_objects(model, objects, steps, [cam], white, export=True))
    assert all("gaussians" not in f for f in simulate_objects(model, [load_object(o, assets, 1, dev()) for o in c.objects], 1, [], white,
                                                               render=False))
    hand = root / "by-hand"
    for f in frames:
        assert f["gaussians"].get_xyz.shape[0] == sum(counts) and torch.equal(f["gaussians"]._xyz, f["means3D"])
        nio.save_gaussians_ply(f["gaussians"], hand / f"{f['step']:03d}.ply")
    gs = [o.gaussians for o in objects]                                      # (mapped into the simulation box by the run)
    opa = torch.cat([g.get_opacity for g in gs], 0)
    with torch.no_grad():
        replayed = dict(render_sequence([hand / f"{f['step']:03d}.ply" for f in frames], [cam], white, 3))
        flush_pending()
        for f in frames[1:]:
            Fs = torch.split(f["deform_grad"].reshape(-1, 3, 3), counts, 0)
            Sy = torch.cat([gc.yardstick_cov(F.contiguous(), g._scaling.detach(), g._rotation.detach(), _svd, o.scaling)
                            for F, g, o in zip(Fs, gs, objects)], 0)
            cov_y = torch.stack([Sy[:, 0, 0], Sy[:, 0, 1], Sy[:, 0, 2], Sy[:, 1, 1], Sy[:, 1, 2], Sy[:, 2, 2]], -1).contiguous()
            yard_img = diff_rasterization(f["means3D"], None, None, cam, white, 3, cov_y, opa, f["shs"])
            flush_pending()
            _pixel_rule(f["images"][0], replayed[f["step"]][0], yard_img, f"two objects, frame {f['step']}")
    # a swapped concatenation or a forgotten modifier would show: the second object's scales carry its 0.6
    last = frames[-1]["gaussians"]
    n0 = counts[0]
    rest_vol = [g._scaling.sum(1) for g in gs]
    detF = torch.linalg.det(frames[-1]["deform_grad"].reshape(-1, 3, 3).double()).abs().log().float()
    want = torch.cat([rest_vol[0], rest_vol[1] + 3 * math.log(0.6)], 0) + detF          # log of the volume: sum of the log-scales
    assert float((last._scaling.sum(1) - want).abs().max()) <= 1e-3
    assert float((last._scaling.sum(1)[n0:] - (rest_vol[1] + detF[n0:])).abs().min()) > 1.0
