"""GPU: SH colours rotated with each Gaussian's own deformation - nm_sh_rotate_polar / rotate_shs_by_deformation against the
fp64 torch formula, its shapes and paths, the rendered statement it exists for (a body moved by the simulator's deformation
gradients and the camera moved with it give the image of the rest pose) and the drivers with `gaussian.rotate_sh`.

Bounds.  Kernel against fp64 (R = the fp64 polar factor of the fp32-rounded F, rows with a defined polar factor only): 4 x the
error of the same computation done by code that exists without the kernel - R32 = U @ Vh from nm_svd3_fwd, then
rotate_shs_per_gaussian_torch in fp32 - on the same rows, floor 1e-6, both relative to the largest fp64 value (the rule of
tests/test_gpu_sh_rotation.py).  R_out against that U @ Vh: 1e-6 absolute, two roundings of three-term dot products of
entries of magnitude <= 1.  Rendered invariance: 4 x the largest pixel difference of the SAME move of the SAME scene at
sh_degree 0, where no coefficient is involved (existing code; pure fp32 reprojection noise)."""
from functools import lru_cache

import numpy as np
import pytest
import torch
import yaml

import svd_cases
from gpu_util import abs_max, dev, measured

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
COMPARED = ("baseline", "rotations", "tie01", "tie12", "tie012", "near_tie", "cond1e3")


def _err(a, ref):
    """max |a - ref| / max |ref| against an fp64 reference (both moved to the CPU)"""
    ref = ref.detach().cpu()
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _svd_fwd(F):
    from neuma_amd import _lib as L
    n = F.shape[0]
    U, s, Vh = torch.empty_like(F), torch.empty(n, 3, device=F.device), torch.empty_like(F)
    L.check(L.lib().nm_svd3_fwd(n, L.ptr(F), L.ptr(U), L.ptr(s), L.ptr(Vh), L.stream_ptr(F.device)), "nm_svd3_fwd")
    return U, Vh


@lru_cache(maxsize=None)
def _families():
    """name -> (F on the GPU, fp64 yardstick, rows with a defined polar factor, U @ Vh of nm_svd3_fwd): computed once"""
    out = {}
    for name, F in svd_cases.families().items():
        yard = svd_cases.yardstick(F)
        Fd = F.to(dev()).contiguous()
        U, Vh = _svd_fwd(Fd)
        out[name] = (Fd, yard, svd_cases.polar_defined(yard), U @ Vh)
    return out


def _coeffs(K, n, seed):
    return torch.randn(K, n, 3, generator=torch.Generator().manual_seed(seed)).to(dev())


def _full(c, R, has_dc):
    from neuma_amd.render.transform_utils import rotate_shs_per_gaussian_torch
    if not has_dc:
        return rotate_shs_per_gaussian_torch(c, R)
    return torch.cat((c[:, :1], rotate_shs_per_gaussian_torch(c[:, 1:], R)), 1)


def _bound_and_error(out, c, R32, R64, rows, has_dc):
    """(error of `out`, bound) on `rows`: the bound is 4 x the fp32 torch path from the existing SVD kernel's rotation"""
    rows_d = rows.to(c.device)
    ref = _full(c[rows_d].double().cpu(), R64[rows], has_dc)
    yard = _err(_full(c[rows_d], R32[rows_d], has_dc), ref)
    return _err(out[rows_d], ref), max(4 * yard, FLOOR), yard


# ------------------------------------------------------------------ 1: kernel against fp64

@pytest.mark.parametrize("has_dc", [0, 1])
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_kernel_matches_the_fp64_formula_on_the_svd_families(deg, has_dc):
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    n = (deg + 1) ** 2 - 1 + has_dc
    for i, (name, (F, yard, keep, R32)) in enumerate(_families().items()):
        K = F.shape[0]
        c = _coeffs(K, n, 1000 * deg + 100 * has_dc + i)
        out, R = rotate_shs_by_deformation(c, F, bool(has_dc), return_rotation=True)
        assert out.data_ptr() != c.data_ptr() and out.shape == c.shape and R.shape == (K, 3, 3)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(R).all()), f"{name}: non-finite output"
        assert abs_max(R, R32) <= 1e-6, f"{name}: R_out is not U @ Vh of nm_svd3_fwd"
        if has_dc:
            assert torch.equal(out[:, 0], c[:, 0]), f"{name}: the DC row is not a copy"
        if name not in COMPARED:
            continue
        share = float(keep.float().mean())
        assert share >= svd_cases.POLAR_KEEP_FLOOR[name], f"{name}: polar_defined keeps {share:.3f}"
        err, bound, yd = _bound_and_error(out, c, R32, yard["R"], keep, has_dc)
        print(f"deg {deg} dc {has_dc} {name}: kept {share:.3f}, fp32 torch from nm_svd3_fwd {yd:.3e}, kernel {err:.3e}, bound {bound:.3e}")
        assert measured(err, f"nm_sh_rotate_polar vs fp64, {name}") <= bound, name


# ------------------------------------------------------------------ 2: shapes

_KMAX = 20_000


@lru_cache(maxsize=None)
def _baseline_case():
    """baseline F (svd_cases._baseline) and N(0,1) coefficients at degree 3 with the DC row, drawn once for the largest K: a
    smaller K takes the leading rows, so a Gaussian has the same inputs in every K"""
    F = svd_cases._baseline(_KMAX, torch.Generator().manual_seed(7)).float().contiguous()
    yard = svd_cases.yardstick(F)
    Fd = F.to(dev())
    U, Vh = _svd_fwd(Fd)
    return Fd, yard, U @ Vh, _coeffs(_KMAX, 16, 8)


@lru_cache(maxsize=None)
def _first_63():
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    F, _, _, c = _baseline_case()
    return rotate_shs_by_deformation(c[:63].contiguous(), F[:63].contiguous(), True, return_rotation=True)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, _KMAX])
def test_shapes_and_independence_of_the_tile(K):
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    F, yard, R32, c = _baseline_case()
    Fk, ck = F[:K].contiguous(), c[:K].contiguous()
    out, R = rotate_shs_by_deformation(ck, Fk, True, return_rotation=True)
    rows = torch.ones(K, dtype=torch.bool)
    err, bound, yd = _bound_and_error(out, ck, R32[:K], yard["R"][:K], rows, 1)
    print(f"K {K}: fp32 torch from nm_svd3_fwd {yd:.3e}, kernel {err:.3e}, bound {bound:.3e}")
    assert measured(err, f"nm_sh_rotate_polar vs fp64, baseline K={K}") <= bound
    assert torch.equal(out[:, 0], ck[:, 0])
    if K >= 63:
        o63, R63 = _first_63()
        assert torch.equal(out[:63], o63) and torch.equal(R[:63], R63), "a Gaussian's result depends on K or on its tile"
    assert torch.equal(rotate_shs_by_deformation(ck, Fk), out), "without R_out the coefficients differ"


def test_unaligned_view_gives_the_same_bits():
    """a view that starts 12 bytes into an allocation takes the 4-byte path"""
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    F, _, _, c = _baseline_case()
    K = 1000
    flat = torch.empty(K * 48 + 3, device=dev())
    view = flat[3:].view(K, 16, 3)
    view.copy_(c[:K])
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    Fk = F[:K].contiguous()
    assert torch.equal(rotate_shs_by_deformation(view, Fk), rotate_shs_by_deformation(c[:K].contiguous(), Fk))
    rest = flat[3:3 + K * 45].view(K, 15, 3)                        # and without the DC row (45 floats per Gaussian)
    assert torch.equal(rotate_shs_by_deformation(rest, Fk, has_dc=False), rotate_shs_by_deformation(rest.clone(), Fk, has_dc=False))


@pytest.mark.parametrize("n,has_dc", [(5, 0), (5, 1), (16, 0), (15, 1), (1, 1), (0, 0), (25, 1)])
def test_other_coefficient_counts_are_an_error(n, has_dc):
    from neuma_amd import _lib as L
    c = torch.zeros(8, max(n, 1), 3, device=dev())
    out = torch.zeros_like(c)
    F = torch.eye(3, device=dev()).expand(8, 3, 3).contiguous()
    rc = L.lib().nm_sh_rotate_polar(8, n, has_dc, L.ptr(F), L.ptr(c), L.ptr(out), None, L.stream_ptr(dev()))
    assert rc != 0 and b"n_coeff" in L.lib().nm_last_error()


def test_in_place_is_refused_and_an_empty_set_is_fine():
    from neuma_amd import _lib as L, NeumaHipError
    from neuma_amd.render.transform_utils import rotate_shs_by_deformation
    c = torch.zeros(8, 16, 3, device=dev())
    F = torch.eye(3, device=dev()).expand(8, 3, 3).contiguous()
    rc = L.lib().nm_sh_rotate_polar(8, 16, 1, L.ptr(F), L.ptr(c), L.ptr(c), None, L.stream_ptr(dev()))
    assert rc != 0 and b"shs_in" in L.lib().nm_last_error()
    assert L.lib().nm_sh_rotate_polar(0, 16, 1, None, None, None, None, L.stream_ptr(dev())) == 0
    one = torch.zeros(8, 1, 3, device=dev())
    assert rotate_shs_by_deformation(one, F) is one
    with pytest.raises(NeumaHipError):
        rotate_shs_by_deformation(c.cpu(), F.cpu())
    with pytest.raises(RuntimeError, match="dependence on F is not propagated"):
        rotate_shs_by_deformation(c, F.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="dependence on F is not propagated"):
        rotate_shs_by_deformation(c.clone().requires_grad_(True), F)
    with torch.no_grad():
        assert torch.equal(rotate_shs_by_deformation(c.clone().requires_grad_(True), F), c)          # identity F, zero colours


# ------------------------------------------------------------------ 3: rendered invariance

def _cov33(c6):
    xx, xy, xz, yy, yz, zz = c6.unbind(-1)
    return torch.stack([torch.stack([xx, xy, xz], -1), torch.stack([xy, yy, yz], -1), torch.stack([xz, yz, zz], -1)], -2)


def _cov6(S):
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).contiguous()


def _shot(gm, means, F, cov6, cam, rotate_sh):
    from neuma_amd.render import flush_pending
    from neuma_amd.tune import diff_rasterization
    img = diff_rasterization(means, F, None, cam, torch.zeros(3, device=dev()), gm.active_sh_degree, cov6, gm.get_opacity,
                             gm.get_features.contiguous(), rotate_sh=rotate_sh)
    flush_pending()
    return img.detach().clone()


def test_rendered_image_is_invariant_when_the_deformation_turns_the_body():
    from test_gpu_sh_rotation import _MOVE_AXIS, _MOVE_DEG, _axis_angle, _cameras, _synth_model
    R64 = _axis_angle(_MOVE_AXIS, _MOVE_DEG)
    R = R64.float().to(dev())
    cam, cam_moved = _cameras(R64)
    Q = _axis_angle((2.0, -1.0, 0.5), 40.0)
    S64 = Q @ torch.diag(torch.tensor([1.3, 0.8, 1.0], dtype=torch.float64)) @ Q.T          # symmetric positive definite
    g0, g3 = _synth_model(0), _synth_model(3)
    K = g3.get_xyz.shape[0]
    means = g3.get_xyz @ R.T
    assert torch.equal(g0.get_xyz, g3.get_xyz)
    cov = g3.get_covariance(1.0)
    # deform_grad = R, and deform_grad = R S with the rest covariance pre-multiplied so that F cov F^T is the rotated one:
    # the polar factor of R S is R, so only R reaches the colours
    Sinv = torch.linalg.inv(S64)
    cov_pre = _cov6((Sinv @ _cov33(cov.double().cpu()) @ Sinv.T).float().to(dev()))
    variants = {"F = R": (R.expand(K, 3, 3).contiguous(), cov),
                "F = R S": ((R64 @ S64).float().to(dev()).expand(K, 3, 3).contiguous(), cov_pre)}
    base0 = _shot(g0, g0.get_xyz, None, cov, cam, False)
    base3 = _shot(g3, g3.get_xyz, None, cov, cam, False)
    assert float(base3.max()) > 0.2, "empty render"
    # yardstick: the same moves at sh_degree 0 through existing code, no coefficient involved; both variants are held to the
    # smaller of the two
    noise = {name: float((_shot(g0, means, F, c6, cam_moved, False) - base0).abs().max()) for name, (F, c6) in variants.items()}
    bound = 4 * min(noise.values())
    for name, (F, c6) in variants.items():
        diff = float((_shot(g3, means, F, c6, cam_moved, True) - base3).abs().max())
        control = float((_shot(g3, means, F, c6, cam_moved, False) - base3).abs().max())
        print(f"{name}: sh0 reprojection noise {noise[name]:.3e}, sh3 rotated {diff:.3e} (bound {bound:.3e}), unrotated control {control:.3e}")
        assert measured(diff, f"sh3 image, body turned by the deformation, {name}, max abs") <= bound
        assert control > 10 * bound, "control: unrotated coefficients must change the image"


# ------------------------------------------------------------------ 4: drivers

def _eval_cfg(path, tmp_path, name, **gaussian):
    from neuma_amd.config import load_config
    from neuma_amd.evaluate import parse_args
    args = parse_args(["-c", str(path), "-vn", name, "-es", "3", "-dv", "r_0", "--result_root", str(tmp_path / "results")])
    cfg = load_config(path)
    for k, val in vars(args).items():
        if k != "config":
            cfg[k] = val
    for k, val in gaussian.items():
        cfg.gaussian[k] = val
    return cfg


def _run_evaluate(cfg):
    from neuma_amd.evaluate import evaluate
    frames = []
    evaluate(cfg, on_frame=lambda step, f: frames.append(dict(means3D=f["means3D"].clone(), deform_grad=f["deform_grad"].clone(),
                                                              image=f["images"]["r_0"].clone())))
    assert len(frames) == 3
    return frames


def _write_init(tmp_path, path):
    """logs/<name>/finetune/init.pt in stage A's layout: evaluate starts from it.  The velocity field spins the body about z
    through its centroid (20 rad/s: about 3 degrees over the three frames), so that F carries a rotation"""
    from neuma_amd.config import load_config
    from neuma_amd.finetune import particle_init_data
    c = load_config(path)
    pos = torch.as_tensor(np.asarray(particle_init_data(c, 4).pos)).float()
    r = pos - pos.mean(0, keepdim=True)
    vel = torch.tensor([0.3, -0.6, 0.1]) + 20.0 * torch.stack([-r[:, 1], r[:, 0], torch.zeros_like(r[:, 0])], 1)
    tune = tmp_path / "logs" / c.name / "finetune"
    tune.mkdir(parents=True, exist_ok=True)
    torch.save({"init_x": pos, "init_v": vel}, tune / "init.pt")


def test_render_entry_point_rotates_once_per_frame(tmp_path):
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import io as nio
    from neuma_amd.config import load_config
    from neuma_amd.finetune import setup
    from neuma_amd.render import flush_pending
    from neuma_amd.render.gaussian_model import GaussianModel
    from neuma_amd.tune import diff_rasterization
    path, _ = _write_experiment(tmp_path, frames=1)
    _write_init(tmp_path, path)
    frames = _run_evaluate(_eval_cfg(path, tmp_path, "rot", rotate_sh=True))
    c = load_config(path)
    env = setup(c, dev(), for_eval=True)
    gm, ds = env["gaussians"], env["dataset"]
    cam = ds.getCameras("r_0", ds.steps[0])
    white = torch.ones(3, device=dev())
    with torch.no_grad():
        # the same renders in the same order as the driver's: a camera sizes and splits its bin lists from what its earlier
        # renders needed, and a different split moves the last bits of a pixel (tests/test_gpu_bind_raster.py: 2e-7)
        diff_rasterization(gm.get_xyz, None, gm, cam, white)
        for f in frames:
            want = diff_rasterization(f["means3D"], f["deform_grad"], gm, cam, white, rotate_sh=True)
            flush_pending()
            assert torch.equal(f["image"], want), "the frame is not what the public operators give for its means3D / deform_grad"
        plain = diff_rasterization(frames[-1]["means3D"], frames[-1]["deform_grad"], gm, cam, white)
        flush_pending()
    moved = float((want - plain).abs().max())
    print(f"last frame with the colours rotated against unrotated: max abs {moved:.3e}")
    assert moved > 1e-4, "the spin must show in the colours: without it the comparison above could not tell the key from no key"
    # ---- sh_degree 0: the key is accepted and changes nothing.  Two runs of the driver cannot be compared bit for bit (the
    #      order of the scatters' float atomics differs from run to run, so their particle states do, measured here too); the
    #      frames of the run WITH the key are therefore held, bit for bit, to what the operators give WITHOUT any rotation for
    #      the same means3D / deform_grad
    raw = tmp_path / "raw"
    full = nio.load_gaussians_ply(raw / "point_cloud.ply", 3)
    g0 = GaussianModel(0)
    g0.set_params(full._xyz, full._features_dc, full._features_rest[:, :0].contiguous(), full._scaling, full._rotation, full._opacity)
    nio.save_gaussians_ply(g0, raw / "point_cloud_sh0.ply")
    cfg0 = yaml.safe_load(path.read_text())
    cfg0["gaussian"].update(sh_degree=0, kernels_path=str(raw / "point_cloud_sh0.ply"))
    cfg0["sim_data_name"] = "tinyball0"
    path0 = tmp_path / "finetune-tiny-sh0.yaml"
    path0.write_text(yaml.safe_dump(cfg0, sort_keys=False))
    with_key = _run_evaluate(_eval_cfg(path0, tmp_path, "sh0-key", rotate_sh=True))
    env0 = setup(load_config(path0), dev(), for_eval=True)
    gm0, ds0 = env0["gaussians"], env0["dataset"]
    assert gm0.active_sh_degree == 0 and gm0.get_features.shape[1] == 1
    cam0 = ds0.getCameras("r_0", ds0.steps[0])
    with torch.no_grad():
        diff_rasterization(gm0.get_xyz, None, gm0, cam0, white)
        for f in with_key:
            plain = diff_rasterization(f["means3D"], f["deform_grad"], gm0, cam0, white)
            flush_pending()
            assert torch.equal(f["image"], plain), "sh_degree 0: the key changed a frame"


def test_inference_entry_point_rotates_the_object_that_asks(tmp_path):
    """two objects, the upper one spinning about z and `gaussian.rotate_sh` on it alone"""
    import shutil
    from PIL import Image
    from test_gpu_entrypoints import _write_experiment
    from neuma_amd import synth
    from neuma_amd.config import load_config
    from neuma_amd.infer import simulate_objects
    from neuma_amd.inference import load_object, main as inference_main
    from neuma_amd.sim import MPMModelBuilder
    path, _ = _write_experiment(tmp_path, frames=1)
    base = yaml.safe_load(path.read_text())
    raw, assets = tmp_path / "raw", tmp_path / "assets"
    w = synth.load_base_weights("plasticine")
    keys = ("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight")
    torch.save({t: {k: torch.tensor(a) for k, a in zip(keys, w[s])} for t, s in (("elasticity", "e"), ("plasticity", "p"))}, raw / "plasticine_0300.pt")
    shutil.copytree(assets / "tinyball", assets / "tinycat")
    for f in (assets / "tinycat").glob("particles.npz"):
        f.unlink()
    steps, omega = 24, 26.0                                          # 24 steps of 1e-3 s at 26 rad/s: 36 degrees of a rigid body

    def obj(name, ckpt, lo, ang, rotate):
        g = dict(sh_degree=3)
        if rotate:
            g["rotate_sh"] = True
        return dict(sim_data_name=name, pretrained_ckpt=str(raw / ckpt), gaussian=g,
                    particle_data=dict(shape=dict(asset_root=None, sort=None, ori_bounds=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                                                  sim_bounds=[[0.25, lo, 0.25], [0.75, lo + 0.5, 0.75]]),
                                       vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=ang), rho=1000.0, clip_bound=0.1),
                    constitution=dict(elasticity=base["constitution"]["elasticity"], plasticity=base["constitution"]["plasticity"], views=["r_0"]))

    def write(name, rotate):
        cfg = dict(gpu=0, seed=42, debug=True, debug_views=["r_0"], resume=False, overwrite=False, denormalize=False, assets_root=str(assets),
                   video_data=dict(base["video_data"], data=dict(base["video_data"]["data"], init_frame=0, used_views=["r_0"])),
                   sim=dict(base["sim"], num_grids=32, eps=6e-7),
                   objects=[obj("tinyball", "jelly_0300.pt", 0.45, [0.0, 0.0, omega], rotate), obj("tinycat", "plasticine_0300.pt", 0.02, [0.0, 0.0, 0.0], False)])
        p = tmp_path / f"{name}.yaml"
        p.write_text(yaml.safe_dump(cfg, sort_keys=False))
        return p

    def png(name, i):
        return np.array(Image.open(tmp_path / "results" / "inference" / f"images_{name}" / f"r_0_{i:03d}.png")).astype(np.int32)

    for name, rotate in (("spin-rot", True), ("spin-plain", False)):
        rc = inference_main(["-c", str(write(name, rotate)), "-s", str(steps), "-vn", name, "-dv", "r_0", "--result_root", str(tmp_path / "results")])
        assert rc in (None, 0)
    assert np.array_equal(png("spin-rot", 0), png("spin-plain", 0)), "the first frame (un-deformed kernels) must be untouched"
    second = int(np.abs(png("spin-rot", 1) - png("spin-plain", 1)).max())
    last = int(np.abs(png("spin-rot", steps) - png("spin-plain", steps)).max())
    print(f"8-bit levels, with the key against without: second frame {second}, last frame {last}")
    assert measured(10 * second, "10 x second-frame difference against the last frame's, key against no key (8-bit levels)") < last
    # ---- the operators by hand: the pack of a frame carries rotated coefficients for the first object only
    c = load_config(tmp_path / "spin-rot.yaml")
    objects = [load_object(o, assets, steps, dev()) for o in c.objects]
    assert [o.rotate_sh for o in objects] == [True, False]
    forced = load_object(load_config(tmp_path / "spin-plain.yaml").objects[1], assets, steps, dev(), rotate_sh=True)      # --rotate_sh
    assert forced.rotate_sh
    model = MPMModelBuilder().parse_cfg(c.sim).finalize(dev(), False)
    from neuma_amd.dataset import CameraDataset
    ds = CameraDataset(c.video_data)
    cam = ds.getCameras("r_0", ds.steps[0])
    loaded = [o.gaussians.get_features.clone() for o in objects]
    k0 = loaded[0].shape[0]
    frames = list(simulate_objects(model, objects, steps, [cam], torch.ones(3, device=dev())))
    assert torch.equal(frames[0]["shs"], torch.cat(loaded, 0)), "frame 0 carries the coefficients as loaded"
    for f in frames[1:]:
        assert torch.equal(f["shs"][k0:], loaded[1]), "the other object's coefficients were touched"
        assert torch.equal(f["shs"][:k0, 0], loaded[0][:, 0]) and not torch.equal(f["shs"][:k0, 1:], loaded[0][:, 1:])
    # the body did turn: polar rotation of the first object's particle F after the run
    n0 = objects[0].init_data.num_particles
    Rp = svd_cases.yardstick(frames[-1]["F"][:n0].float())["R"]
    ang = torch.rad2deg(torch.acos(((Rp.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)))
    print(f"rotation of the spinning object's particles after {steps} steps: median {float(ang.median()):.1f} degrees")
    assert float(ang.median()) >= 20.0


def test_finetune_refuses_the_key(tmp_path):
    from neuma_amd.config import load_config
    from neuma_amd.finetune import finetune
    path = tmp_path / "finetune-rot.yaml"
    path.write_text(yaml.safe_dump(dict(gpu=0, seed=42, root=str(tmp_path / "logs"), name="rot", gaussian=dict(sh_degree=3, rotate_sh=True))))
    with pytest.raises(NotImplementedError, match=r"gaussian\.rotate_sh"):
        finetune(load_config(path))
    assert not (tmp_path / "logs").exists()
