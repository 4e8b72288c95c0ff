"""GPU: SH colour coefficients rotated with the Gaussians - nm_sh_rotate / nm_sh_rotate_backward against the fp64 torch
formula (sh_rotation_matrices), the rendered statement (moving the Gaussians and the camera by one rigid motion leaves the
image unchanged), the registration loop at sh_degree 3 against the autograd path, recovery of a known transform from targets
rendered with rotated colours, and the entry point with `register.rotate_sh: true`.

Bounds.  Kernel against fp64: 4 x the error of the same computation done by torch in fp32 (rotate_shs_torch and its autograd)
against fp64, floor 1e-6, both relative to the largest fp64 value (the rule of the classical laws).  Rendered
invariance: 4 x the largest pixel difference of the SAME rigid move of the SAME scene at sh_degree 0, where no coefficient
is rotated (existing code; pure fp32 reprojection noise).  Loop: the bounds of tests/test_gpu_regist.py's two loop tests."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from gpu_util import dev, measured, rel_max

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FLOOR = 1e-6


def _rot(seed, device=None, dtype=torch.float32):
    from neuma_amd.regist import quat_to_rotmat
    q = torch.randn(4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return quat_to_rotmat(q / q.norm()).to(dtype).to(device or dev())


def _axis_angle(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    t = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def _err(a, ref):
    """max |a - ref| / max |ref| against an fp64 reference"""
    return float((a.detach().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _full64(c64, R64, has_dc):
    from neuma_amd.render.transform_utils import rotate_shs_torch
    if not has_dc:
        return rotate_shs_torch(c64, R64)
    return torch.cat((c64[:, :1], rotate_shs_torch(c64[:, 1:], R64)), 1)


def _full32(c32, R32, has_dc):
    return _full64(c32, R32, has_dc)


# ------------------------------------------------------------------ forward

@pytest.mark.parametrize("K", [1, 257, 200_000])
@pytest.mark.parametrize("has_dc", [0, 1])
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_forward_matches_the_fp64_formula(deg, has_dc, K):
    from neuma_amd.render.transform_utils import sh_rotate
    n = (deg + 1) ** 2 - 1 + has_dc
    gen = torch.Generator().manual_seed(100 * deg + 10 * has_dc + 1)
    c = torch.randn(K, n, 3, generator=gen).to(dev())
    R = _rot(deg + 7)
    ref = _full64(c.double(), R.double(), has_dc)
    yard = _err(_full32(c, R, has_dc), ref)
    bound = max(4 * yard, FLOOR)
    out = sh_rotate(c, R.reshape(9).contiguous(), bool(has_dc))
    print(f"deg {deg} dc {has_dc} K {K}: fp32 torch {yard:.3e}")
    assert measured(_err(out, ref), "sh_rotate vs fp64 (out of place)") <= bound
    if has_dc:
        assert torch.equal(out[:, 0], c[:, 0]), "DC row is not a copy"
    inplace = c.clone()
    got = sh_rotate(inplace, R.reshape(9).contiguous(), bool(has_dc), out=inplace)
    assert got.data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace, out), "in place and out of place differ"


def test_forward_from_an_unaligned_view():
    """a slice that starts 12 bytes into an allocation takes the 4-byte path and gives the same bits"""
    from neuma_amd.render.transform_utils import sh_rotate
    gen = torch.Generator().manual_seed(5)
    K = 1000
    flat = torch.randn(K * 45 + 3, generator=gen).to(dev())
    c = flat[3:].view(K, 15, 3)
    assert c.data_ptr() % 16 != 0
    R9 = _rot(3).reshape(9).contiguous()
    assert torch.equal(sh_rotate(c, R9, False), sh_rotate(c.clone(), R9, False))


@pytest.mark.parametrize("n,has_dc", [(5, 0), (5, 1), (16, 0), (15, 1), (1, 1), (0, 0), (25, 1)])
def test_other_coefficient_counts_are_an_error(n, has_dc):
    from neuma_amd import _lib as L
    c = torch.zeros(8, max(n, 1), 3, device=dev())
    R9 = torch.eye(3, device=dev()).reshape(9).contiguous()
    rc = L.lib().nm_sh_rotate(8, n, has_dc, L.ptr(R9), L.ptr(c), L.ptr(c), L.stream_ptr(dev()))
    assert rc != 0 and b"n_coeff" in L.lib().nm_last_error()
    ws = torch.empty(int(L.lib().nm_sh_rotate_bwd_workspace(8)), dtype=torch.uint8, device=dev())
    rc = L.lib().nm_sh_rotate_backward(8, n, has_dc, L.ptr(R9), L.ptr(c), L.ptr(c), L.ptr(R9.clone()), None, L.ptr(ws), ws.numel(),
                                       L.stream_ptr(dev()))
    assert rc != 0


# ------------------------------------------------------------------ backward

@pytest.mark.parametrize("K", [257, 200_000])
@pytest.mark.parametrize("has_dc", [0, 1])
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_backward_matches_fp64_autograd_and_is_reproducible(deg, has_dc, K):
    from neuma_amd.render.transform_utils import sh_rotate_backward
    n = (deg + 1) ** 2 - 1 + has_dc
    gen = torch.Generator().manual_seed(200 * deg + 10 * has_dc + 3)
    c = torch.randn(K, n, 3, generator=gen).to(dev())
    go = torch.randn(K, n, 3, generator=gen).to(dev())
    R = _rot(deg + 17)

    def autograd(dtype):
        cc, RR = c.to(dtype).requires_grad_(True), R.to(dtype).requires_grad_(True)
        (_full64(cc, RR, has_dc) * go.to(dtype)).sum().backward()
        return RR.grad, cc.grad

    dR64, dc64 = autograd(torch.float64)
    dR32, dc32 = autograd(torch.float32)
    bound_R = max(4 * _err(dR32, dR64), FLOOR)
    bound_c = max(4 * _err(dc32, dc64), FLOOR)
    R9 = R.reshape(9).contiguous()
    start = torch.linspace(-2.0, 3.0, 9, device=dev())                    # dL_dR is ADDED to what the array holds
    d1 = start.clone()
    g1 = sh_rotate_backward(c, R9, bool(has_dc), go, d1)
    d2 = start.clone()
    g2 = sh_rotate_backward(c, R9, bool(has_dc), go, d2)
    assert torch.equal(d1, d2) and torch.equal(g1, g2), "two identical calls differ"
    err_R = float((d1.double().reshape(3, 3) - (start.double().reshape(3, 3) + dR64)).abs().max()) / float(dR64.abs().max())
    assert measured(err_R, "dL_dR vs fp64 autograd") <= bound_R
    assert measured(_err(g1, dc64), "dL_dshs_in vs fp64 autograd") <= bound_c
    d3 = start.clone()
    assert sh_rotate_backward(c, R9, bool(has_dc), go, d3, want_dshs=False) is None       # dL_dshs_in = NULL
    assert torch.equal(d3, d1)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_autograd_function_gives_the_same_numbers(deg):
    from neuma_amd.render.transform_utils import sh_rotate, sh_rotate_backward, transform_shs_by_quat, transform_shs_by_rotmat
    from neuma_amd.regist import rotmat_to_quat
    K, n = 5000, (deg + 1) ** 2 - 1
    gen = torch.Generator().manual_seed(31 + deg)
    c = torch.randn(K, n, 3, generator=gen).to(dev())
    go = torch.randn(K, n, 3, generator=gen).to(dev())
    R = _rot(40 + deg)
    cc, RR = c.clone().requires_grad_(True), R.clone().requires_grad_(True)
    out = transform_shs_by_rotmat(cc, RR)
    assert out.data_ptr() != cc.data_ptr()
    (out * go).sum().backward()
    R9 = R.reshape(9).contiguous()
    dR = torch.zeros(9, device=dev())
    dc = sh_rotate_backward(c, R9, False, go, dR)
    assert torch.equal(out.detach(), sh_rotate(c, R9, False))
    assert torch.equal(RR.grad.reshape(9), dR) and torch.equal(cc.grad, dc)
    ref = _full64(c.double(), R.double(), 0)
    by_quat = transform_shs_by_quat(c, rotmat_to_quat(R))
    assert measured(_err(by_quat, ref), "transform_shs_by_quat vs fp64") <= 1e-5       # (R -> q -> R in fp32 on the way)
    one = torch.randn(K, 1, 3, device=dev())
    assert transform_shs_by_rotmat(one, R) is one


# ------------------------------------------------------------------ rendered invariance

_MOVE_AXIS, _MOVE_DEG = (1.0, 2.0, 3.0), 25.0        # the rigid move: 25 degrees about (1, 2, 3), about the world origin
# SH amplitude.  Reprojection noise is sum_i dw_i c_i with sum_i dw_i ~ 0: it scales with the SPREAD of the colours among the
# Gaussians a pixel blends.  Every basis function has rms 1 / sqrt(4 pi) over the sphere, so N(0, a_j) coefficients give a spread
# of sqrt(sum_j a_j^2 / 4 pi): 0.085 for the DC row alone (a = 0.3, the sh-0 yardstick) and 4 x that with all 16 rows at 0.3 -
# the yardstick would then measure a scene with a quarter of the contrast (measured so: noise 3.6e-4 at sh 0, 1.85e-3 at sh 3
# with the coefficients rotated, 0.14 unrotated).  The rows above the DC row are therefore scaled by 0.25 (a = 0.075): spread
# sqrt(1 + 15/16) = 1.4 x the yardstick's, inside the factor 4, while the unrotated control stays two orders above the noise.
_REST_SCALE = 0.25


def _synth_model(sh, K=20000, seed=0):
    """the `tiny` synth scene: geometry and opacity do not depend on `sh` (they are drawn first), DC row ~ N(0, 0.3)
    (synth.make_scene's own amplitude), the rows above it scaled by _REST_SCALE"""
    from neuma_amd import synth
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = synth.make_scene("tiny", seed=seed, override=dict(K=K, sh=sh))
    d = dev()
    gm = GaussianModel(sh)
    c = torch.tensor(sc.g_sh, device=d)
    gm.set_params(torch.tensor(sc.g_xyz, device=d), c[:, :1].contiguous(), (_REST_SCALE * c[:, 1:]).contiguous(),
                  torch.tensor(sc.g_logscale, device=d), torch.tensor(sc.g_rot, device=d), torch.tensor(sc.g_opacity_logit, device=d))
    return gm


def _render(gm, cam):
    from neuma_amd.render import flush_pending, get_rasterizer
    rast = get_rasterizer(cam, gm.active_sh_degree, False, torch.zeros(3, device=dev()))
    img, _ = rast(means3D=gm.get_xyz, means2D=torch.zeros_like(gm.get_xyz), opacities=gm.get_opacity, shs=gm.get_features.contiguous(),
                  colors_precomp=None, cov3D_precomp=gm.get_covariance(1.0))
    flush_pending()
    return img.detach().clone()


def _cameras(R64, W=480, H=270):
    from neuma_amd import synth
    eye, target, up = np.array([1.2, 0.9, 1.7]), np.array([0.5, 0.5, 0.5]), np.array([0.0, -1.0, 0.0])
    Rn = R64.numpy()
    fov = math.radians(40.0)
    return (synth.SynthCamera(W, H, fov, eye, target, up, device=dev()),
            synth.SynthCamera(W, H, fov, Rn @ eye, Rn @ target, Rn @ up, device=dev()))


def test_rendered_image_is_invariant_under_a_joint_rigid_move():
    from neuma_amd.render.transform_utils import rotate_gaussians, rotate_transform
    R64 = _axis_angle(_MOVE_AXIS, _MOVE_DEG)
    R = R64.float().to(dev())
    cam, cam_moved = _cameras(R64)
    # yardstick: the same move of the same scene at sh_degree 0 (rotate_gaussians touches no coefficient there)
    g0 = _synth_model(0)
    base0 = _render(g0, cam)
    rotate_gaussians(g0, R)
    noise = float((_render(g0, cam_moved) - base0).abs().max())
    bound = 4 * noise
    g3 = _synth_model(3)
    base3 = _render(g3, cam)
    assert float(base3.max()) > 0.2, "empty render"
    rest = g3._features_rest.clone()
    rotate_gaussians(g3, R)
    assert g3._features_rest.data_ptr() != rest.data_ptr()
    diff = float((_render(g3, cam_moved) - base3).abs().max())
    # control: the same move with the coefficients left as they were
    g3._features_rest = rest
    control = float((_render(g3, cam_moved) - base3).abs().max())
    print(f"rendered invariance: sh0 reprojection noise {noise:.3e}, sh3 moved {diff:.3e} (bound {bound:.3e}), unrotated control {control:.3e}")
    assert measured(diff, "sh3 image after a joint move, max abs") <= bound
    assert control > 10 * bound, "control: unrotated coefficients must change the image"
    # rotate_transform is the same move of positions and orientations
    g = _synth_model(3)
    p, q = rotate_transform(g.get_xyz, g.get_rotation, R)
    assert torch.equal(p, g3._xyz) and torch.equal(q, g3._rotation)


# ------------------------------------------------------------------ the loop at sh_degree 3

def _scene(K=20000, W=480, H=270, V=3, seed=0, sh=3):
    from neuma_amd import synth
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = synth.make_scene("tiny", seed=seed, override=dict(K=K, W=W, H=H, V=V, sh=sh))
    d = dev()
    gm = GaussianModel(sh)
    c = torch.tensor(sc.g_sh, device=d)
    rot = torch.tensor(sc.g_rot, device=d) * 1.7                       # not normalised, as a PLY may hold them
    gm.set_params(torch.tensor(sc.g_xyz, device=d), c[:, :1].contiguous(), c[:, 1:].contiguous(),
                  torch.tensor(sc.g_logscale, device=d), rot.contiguous(), torch.tensor(sc.g_opacity_logit, device=d))
    return gm, synth.ring_cameras(V, W, H, device=d)


def _ground_truth(gm, cams, bg, r6, t, s):
    """targets rendered at a known transform WITH the colours rotated by it"""
    from test_gpu_regist import _reg_cfg
    from neuma_amd.regist import NativeRegistration, Register, pack_params, regist_apply
    from neuma_amd.render import raster_forward_raw
    reg = Register(_reg_cfg([0, 0, 0], t, [s]), device=dev())
    with torch.no_grad():
        reg.r.copy_(r6)
    reg.training_setup()
    run = NativeRegistration(reg, gm, cams, [torch.zeros(3, c.image_height, c.image_width, device=dev()) for c in cams], bg)
    assert run.rotate_sh
    _, _, params = pack_params(reg, run.origin)
    m, c6 = regist_apply(run.xyz, run.ls, run.rot, params, 1.0)
    sh = run._rotated_sh(params)
    return [raster_forward_raw(cam, m, sh, None, run.op, c6)[0].clone() for cam in run.cams]


def test_native_loop_matches_the_autograd_path_at_sh3():
    from test_gpu_regist import _reg_cfg
    from neuma_amd.regist import NativeRegistration, Register, euler_to_quat, quat_to_rot6d, regist_step_torch
    from neuma_amd.render import flush_pending
    from neuma_amd.render.transform_utils import rotate_shs_torch
    gm, cams = _scene()
    bg = torch.zeros(3, device=dev())
    true_r6 = quat_to_rot6d(euler_to_quat(torch.tensor([4.0, -3.0, 2.0], device=dev()) * math.pi / 180))
    gts = _ground_truth(gm, cams, bg, true_r6, [0.01, -0.02, 0.015], 1.03)
    lam = 0.2
    cfg = _reg_cfg([0, 0, 0], [0.0, 0.0, 0.0], [1.0], lam=lam)
    a, b = Register(cfg, device=dev()), Register(cfg, device=dev())
    a.training_setup(); b.training_setup()
    run = NativeRegistration(a, gm, cams, gts, bg, lambda_ssim=lam, num_iter=20)
    hist_t = []
    for _ in range(20):
        run.step()
        loss, _ = regist_step_torch(b, gm, cams, gts, bg, lambda_ssim=lam)
        hist_t.append(float(loss))
    flush_pending()
    hist_n = run.losses()
    assert rel_max(torch.tensor(hist_n), torch.tensor(hist_t)) <= 1e-4
    for name in ("r", "t", "s"):
        assert rel_max(getattr(a, name).detach(), getattr(b, name).detach()) <= 1e-5, name
    assert abs(hist_n[-1]) < abs(hist_n[0])
    # the Gaussians of the last forward pass carry the colours rotated by that pass's R
    m, ls, rq, f_rest = run.transformed(with_f_rest=True)
    R_last = run.last_params[0:9].reshape(3, 3)
    ref = rotate_shs_torch(gm._features_rest.double(), R_last.double())
    assert measured(_err(f_rest, ref), "transformed() f_rest vs fp64") <= max(4 * _err(rotate_shs_torch(gm._features_rest, R_last), ref), FLOOR)
    assert len(run.transformed()) == 3


def test_recovers_a_known_transform_from_targets_with_rotated_colours():
    from test_gpu_regist import _reg_cfg
    from neuma_amd.regist import NativeRegistration, Register, euler_to_quat, quat_to_rot6d, rot6d_to_rotmat
    from neuma_amd.render import flush_pending
    torch.manual_seed(0)
    gm, cams = _scene()
    bg = torch.zeros(3, device=dev())
    true_e, true_t, true_s = [3.0, -2.0, 4.0], [0.004, -0.006, 0.005], 1.0
    true_r6 = quat_to_rot6d(euler_to_quat(torch.tensor(true_e, device=dev()) * math.pi / 180))
    gts = _ground_truth(gm, cams, bg, true_r6, true_t, true_s)
    cfg = _reg_cfg([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.05], lr=(6e-3, 1.5e-3, 4e-3), lam=0.0)
    cfg.scheduler = dict(max_steps=600, learning_rate_alpha=0.05)
    reg = Register(cfg, device=dev())
    reg.training_setup()
    run = NativeRegistration(reg, gm, cams, gts, bg, num_iter=600)
    for _ in range(600):
        run.step()
    flush_pending()
    R = rot6d_to_rotmat(reg.r.detach()).double()
    Rt = rot6d_to_rotmat(true_r6).double()
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(R.T @ Rt)) - 1) / 2))))
    dt = float((reg.t.detach().double().cpu() - torch.tensor(true_t, dtype=torch.float64)).norm())
    ds = abs(float(reg.s.detach()[0]) - true_s)
    losses = run.losses()
    print(f"recovery at sh 3: angle {ang:.3f} deg, |dt| {dt:.5f}, |ds| {ds:.5f}, loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert measured(ang, "rotation error deg") <= 1.0
    assert measured(dt, "translation error") <= 0.003
    assert measured(ds, "scale error") <= 0.01
    assert losses[-1] < 0.2 * losses[0]


# ------------------------------------------------------------------ the entry point

def test_entry_point_rotates_the_colours_when_asked(tmp_path):
    from test_gpu_regist import _run, _write_regist_experiment
    from neuma_amd import io as nio
    from neuma_amd.prepare import prepare_simulation_data
    from neuma_amd.render.transform_utils import rotate_shs_torch
    path, cfg = _write_regist_experiment(tmp_path, sh_degree=1, num_iter=30)
    cfg["register"]["rotate_sh"] = True
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    p = _run(path)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    root = tmp_path / "assets" / "regbox"
    loaded = nio.load_gaussians_ply(tmp_path / "raw" / "point_cloud.ply", 1)
    g = nio.load_gaussians_ply(root / "registered_kernels.ply", 1)
    assert g.active_sh_degree == 1 and g._features_rest.shape == (3000, 3, 3)
    assert torch.equal(g._features_dc, loaded._features_dc)
    # R of the last forward pass from the geometry the same file holds (orthogonal Procrustes in fp64): x' = s R (x - o) + t
    X = loaded._xyz.double() - loaded._xyz.double().mean(0, keepdim=True)
    Y = g._xyz.double() - g._xyz.double().mean(0, keepdim=True)
    U, _, Vh = torch.linalg.svd(Y.T @ X)
    R_last = U @ torch.diag(torch.tensor([1.0, 1.0, float(torch.det(U @ Vh))], dtype=torch.float64)) @ Vh
    z = np.load(root / "registered_params.npz")
    step = float(np.abs(R_last.numpy() - z["r"]).max())
    assert step < 1e-2, "the saved Gaussians are those of the last forward pass, one optimizer step behind r"
    ref = rotate_shs_torch(loaded._features_rest.double(), R_last)
    yard = _err(rotate_shs_torch(loaded._features_rest, R_last.float()), ref)
    assert measured(_err(g._features_rest, ref), "registered f_rest vs D(R_last) f_rest") <= max(4 * yard, FLOOR)
    assert _err(loaded._features_rest, ref) > 1e-3, "the rotation must have changed the coefficients"
    out = tmp_path / "prep"
    prepare_simulation_data(save_dir=out, kernels_path=root / "registered_kernels.ply", particles_path=root / "registered_particles.ply",
                            sh_degree=1, particles_downsample_factor=1, device=dev())
    assert all((out / n).is_file() for n in ("kernels.ply", "particles.ply", "bindings.pt"))


def test_entry_point_refusal_names_the_key(tmp_path):
    from test_gpu_regist import _write_regist_experiment
    from neuma_amd.config import load_config
    from neuma_amd.regist import regist_gaussians
    path, _ = _write_regist_experiment(tmp_path, sh_degree=1, num_iter=2)
    with pytest.raises(NotImplementedError, match=r"sh_degree > 0.*register\.rotate_sh"):
        regist_gaussians(load_config(path))
