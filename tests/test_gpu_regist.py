"""GPU: Gaussian registration (python -m neuma_amd.regist, experiments/regist.py) - nm_regist_apply / nm_regist_backward against
the reference's transform chain (tests/golden/regist/regist_transform.npz), nm_ssim_loss against loss_utils.ssim
(tests/golden/regist/ssim.npz) and an fp64 torch restatement at 1080p, the native loop against the torch autograd path, recovery
of a known transform, and the entry point on a small dataset in the reference's layout."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from gpu_util import dev, measured, rel_max

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "regist"
sys.path.insert(0, str(GOLD.parent))
import regist_inputs as ri  # noqa: E402  (the fixtures' inputs, rebuilt bit for bit)


def _t(a, d=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=d or dev())


# ------------------------------------------------------------------ fp64 torch restatements

def _window64(device):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).to(device)[None, None].expand(3, 1, 11, 11).contiguous()


def ssim64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """loss_utils.py:35-66 in fp64 (grouped conv2d, zero padding 5, sigma^2 = E[x^2] - mu^2)."""
    w = _window64(a.device)
    c = lambda x: F.conv2d(x[None], w, padding=5, groups=3)[0]
    mu1, mu2 = c(a), c(b)
    s1, s2, s12 = c(a * a) - mu1 ** 2, c(b * b) - mu2 ** 2, c(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()


def _ssim_native(img, gt, weight, loss=None, grad=None):
    from neuma_amd import _lib as L
    lib = L.lib()
    h, w = img.shape[-2:]
    loss = torch.zeros((), dtype=torch.float32, device=img.device) if loss is None else loss
    ws = torch.empty(int(lib.nm_ssim_workspace(h, w)), dtype=torch.uint8, device=img.device)
    L.check(lib.nm_ssim_loss(float(weight), h, w, L.ptr(img), L.ptr(gt), L.ptr(loss), L.ptr(grad), L.ptr(ws), ws.numel(),
                             L.stream_ptr(img.device)), "nm_ssim_loss")
    return loss, grad


# ------------------------------------------------------------------ 1. / 2. transform and its adjoint

@pytest.mark.parametrize("case", ["c0", "c1"])
def test_regist_apply_matches_the_reference_chain(case):
    from neuma_amd.regist import regist_apply
    z = np.load(GOLD / "regist_transform.npz")
    g = lambda k: z[f"{case}_{k}"]
    inp = ri.transform_inputs()
    params = _t(np.concatenate([g("R").ravel(), g("q_R"), g("s"), g("t"), g("o").ravel()]))
    means, cov, ls, rq = regist_apply(_t(inp["xyz"]), _t(inp["log_scales"]), _t(inp["rot"]), params, float(g("scaling_modifier")[0]),
                                      want_params=True)
    torch.cuda.synchronize()
    rows = slice(0, None, ri.ROW_STRIDE)           # the rows the fixture holds (every 16th Gaussian)
    assert rel_max(means[rows], torch.tensor(g("means3D"))) <= 2e-6
    assert rel_max(cov[rows], torch.tensor(g("cov6"))) <= 2e-6
    assert rel_max(ls[rows], torch.tensor(g("out_log_scales"))) <= 2e-6
    assert rel_max(rq[rows], torch.tensor(g("out_rot"))) <= 2e-6


@pytest.mark.parametrize("case", ["c0", "c1"])
def test_regist_backward_matches_fp64_autograd_and_is_reproducible(case):
    from neuma_amd.regist import regist_backward
    z = np.load(GOLD / "regist_transform.npz")
    g = lambda k: z[f"{case}_{k}"]
    inp = ri.transform_inputs()
    params = _t(np.concatenate([g("R").ravel(), g("q_R"), g("s"), g("t"), g("o").ravel()]))
    args = (_t(inp["xyz"]), _t(inp["log_scales"]), _t(inp["rot"]), params, float(g("scaling_modifier")[0]), _t(inp["dL_dmeans3D"]),
            _t(inp["dL_dcov6"]))
    d1 = regist_backward(*args, torch.zeros(17, device=dev()))
    d2 = regist_backward(*args, torch.zeros(17, device=dev()))
    torch.cuda.synchronize()
    assert torch.equal(d1, d2), "two identical calls differ"
    for name, sl in (("dR", slice(0, 9)), ("dq_R", slice(9, 13)), ("ds", slice(13, 14)), ("dt", slice(14, 17))):
        assert rel_max(d1[sl], torch.tensor(g(name)).reshape(-1)) <= 1e-5, name
    acc = regist_backward(*args, d1.clone())        # += semantics
    torch.cuda.synchronize()
    assert rel_max(acc, 2 * d1.double()) <= 1e-6


# ------------------------------------------------------------------ 3. SSIM

@pytest.mark.parametrize("tag", ["16x16", "37x53", "135x240"])
def test_ssim_matches_the_reference(tag):
    from neuma_amd.tune import ssim
    z = np.load(GOLD / "ssim.npz")
    h, w = (int(n) for n in tag.split("x"))
    a, b = ri.ssim_images(h, w)
    a, b = _t(a).requires_grad_(True), _t(b)
    rows = torch.tensor(ri.ssim_rows(h))
    v = ssim(a, b)
    v.backward()
    v = float(v.detach())
    assert measured(abs(v - float(z[f"ssim64_{tag}"])), "ssim value vs fp64") <= 2e-6
    assert measured(abs(v - float(z[f"ssim32_{tag}"])), "ssim value vs fp32 reference") <= 2e-6
    assert rel_max(a.grad.cpu()[:, rows], torch.tensor(z[f"grad64_{tag}"])) <= 1e-4
    assert rel_max(a.grad.cpu()[:, rows], torch.tensor(z[f"grad32_{tag}"])) <= 1e-4


def test_ssim_1080p_against_fp64_restatement():
    gen = torch.Generator(device="cpu").manual_seed(5)
    base = torch.rand(3, 1080, 1920, generator=gen)
    a = (0.7 * base + 0.3 * torch.rand(3, 1080, 1920, generator=gen)).to(dev())
    b = (base + 0.05 * torch.randn(3, 1080, 1920, generator=gen)).clamp(0, 1).to(dev())
    grad = torch.zeros_like(a)
    loss, grad = _ssim_native(a, b, 1.0, grad=grad)
    a64 = a.double().requires_grad_(True)
    ref = 1.0 - ssim64(a64, b.double())
    ref.backward()
    assert measured(abs(float(loss) - float(ref)), "1-ssim 1080p vs fp64") <= 2e-6
    assert rel_max(grad, a64.grad) <= 1e-4
    loss2, grad2 = _ssim_native(a, b, 1.0, grad=torch.zeros_like(a))
    assert torch.equal(loss, loss2), "loss value not deterministic"


def test_ssim_composes_with_pixel_loss():
    from neuma_amd import _lib as L
    lam = 0.1
    gen = torch.Generator(device="cpu").manual_seed(9)
    a = torch.rand(3, 135, 240, generator=gen)
    b = (a + 0.1 * torch.randn(3, 135, 240, generator=gen)).clamp(0, 1).to(dev())
    a = a.to(dev())
    loss = torch.zeros((), dtype=torch.float32, device=dev())
    grad = torch.empty_like(a)
    L.check(L.lib().nm_pixel_loss(0, 1.0 - lam, 135, 240, 0, 0, L.ptr(a), L.ptr(b), L.ptr(loss), L.ptr(grad), L.stream_ptr(a.device)))
    _ssim_native(a, b, lam, loss=loss, grad=grad)
    a64 = a.double().requires_grad_(True)
    ref = (1 - lam) * (a64 - b.double()).abs().mean() + lam * (1 - ssim64(a64, b.double()))
    ref.backward()
    assert measured(abs(float(loss) - float(ref)) / float(ref), "composed loss rel") <= 2e-6
    assert rel_max(grad, a64.grad) <= 1e-4


# ------------------------------------------------------------------ 4. / 5. the loop

def _scene(K=20000, W=480, H=270, V=3, seed=0):
    from neuma_amd import synth
    from neuma_amd.render.gaussian_model import GaussianModel
    sc = synth.make_scene("tiny", seed=seed, override=dict(K=K, W=W, H=H, V=V, sh=0))
    d = dev()
    gm = GaussianModel(0)
    sh = torch.tensor(sc.g_sh, device=d)
    rot = torch.tensor(sc.g_rot, device=d) * 1.7                       # not normalised, as a PLY may hold them
    gm.set_params(torch.tensor(sc.g_xyz, device=d), sh[:, :1].contiguous(), sh[:, 1:].contiguous(),
                  torch.tensor(sc.g_logscale, device=d), rot.contiguous(), torch.tensor(sc.g_opacity_logit, device=d))
    cams = synth.ring_cameras(V, W, H, device=d)
    return gm, cams


def _reg_cfg(init_r, init_t, init_s, lr=(1e-4, 5e-5, 1e-5), lam=0.0):
    from neuma_amd.config import Cfg
    return Cfg(INIT_R=list(init_r), INIT_T=list(init_t), INIT_S=list(init_s), lr_r=lr[0], lr_t=lr[1], lr_s=lr[2],
               lambda_ssim_loss=lam, scheduler=dict(max_steps=20000, learning_rate_alpha=0.01))


def _ground_truth(gm, cams, bg, r6, t, s, mask, mod=1.0):
    from neuma_amd.regist import NativeRegistration, Register
    reg = Register(_reg_cfg([0, 0, 0], t, [s]), device=dev())
    with torch.no_grad():
        reg.r.copy_(r6)
    reg.training_setup()
    run = NativeRegistration(reg, gm, cams, [torch.zeros(3, c.image_height, c.image_width, device=dev()) for c in cams], bg,
                             force_mask_data=mask, scaling_modifier=mod)
    from neuma_amd.render import raster_forward_raw
    from neuma_amd.regist import pack_params, regist_apply
    _, _, params = pack_params(reg, run.origin)
    m, c6 = regist_apply(run.xyz, run.ls, run.rot, params, mod)
    return [raster_forward_raw(cam, m, run.sh, run.cp, run.op, c6)[0].clone() for cam in run.cams]


@pytest.mark.parametrize("mask", [False, True])
def test_native_loop_matches_the_autograd_path(mask):
    from neuma_amd.regist import NativeRegistration, Register, regist_step_torch, rot6d_to_rotmat, euler_to_quat, quat_to_rot6d
    from neuma_amd.render import flush_pending
    gm, cams = _scene()
    bg = torch.zeros(3, device=dev())
    true_r6 = quat_to_rot6d(euler_to_quat(torch.tensor([4.0, -3.0, 2.0], device=dev()) * math.pi / 180))
    gts = _ground_truth(gm, cams, bg, true_r6, [0.01, -0.02, 0.015], 1.03, mask)
    lam = 0.2
    cfg = _reg_cfg([0, 0, 0], [0.0, 0.0, 0.0], [1.0], lam=lam)
    a, b = Register(cfg, device=dev()), Register(cfg, device=dev())
    a.training_setup(); b.training_setup()
    run = NativeRegistration(a, gm, cams, gts, bg, lambda_ssim=lam, force_mask_data=mask, num_iter=20)
    hist_t = []
    for _ in range(20):
        run.step()
        loss, _ = regist_step_torch(b, gm, cams, gts, bg, lambda_ssim=lam, force_mask_data=mask)
        hist_t.append(float(loss))
    flush_pending()
    hist_n = run.losses()
    assert rel_max(torch.tensor(hist_n), torch.tensor(hist_t)) <= 1e-4
    for name in ("r", "t", "s"):
        assert rel_max(getattr(a, name).detach(), getattr(b, name).detach()) <= 1e-5, name
    assert abs(hist_n[-1]) < abs(hist_n[0])


def test_recovers_a_known_transform():
    from neuma_amd.regist import NativeRegistration, Register, euler_to_quat, quat_to_rot6d, rot6d_to_rotmat
    from neuma_amd.render import flush_pending
    torch.manual_seed(0)
    gm, cams = _scene()
    bg = torch.zeros(3, device=dev())
    true_e, true_t, true_s = [3.0, -2.0, 4.0], [0.004, -0.006, 0.005], 1.0
    true_r6 = quat_to_rot6d(euler_to_quat(torch.tensor(true_e, device=dev()) * math.pi / 180))
    gts = _ground_truth(gm, cams, bg, true_r6, true_t, true_s, False)
    # start ~5 degrees, 2 % of the scene size and 5 % of scale away; raised learning rates, fixed number of iterations
    # (RAdam's rectification keeps the early steps at a fraction of the rate: the rates are sized for that)
    cfg = _reg_cfg([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.05], lr=(6e-3, 1.5e-3, 4e-3), lam=0.0)
    cfg.scheduler = dict(max_steps=600, learning_rate_alpha=0.05)
    reg = Register(cfg, device=dev())
    reg.training_setup()
    run = NativeRegistration(reg, gm, cams, gts, bg, force_mask_data=False, num_iter=600)
    for _ in range(600):
        run.step()
    flush_pending()
    R = rot6d_to_rotmat(reg.r.detach()).double()
    Rt = rot6d_to_rotmat(true_r6).double()
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(R.T @ Rt)) - 1) / 2))))
    dt = float((reg.t.detach().double().cpu() - torch.tensor(true_t, dtype=torch.float64)).norm())
    ds = abs(float(reg.s.detach()[0]) - true_s)
    losses = run.losses()
    print(f"recovery: angle {ang:.3f} deg, |dt| {dt:.5f}, |ds| {ds:.5f}, loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    # start: 5.4 degrees, |dt| 0.0088 (1.7 % of the scene), |ds| 0.05
    assert measured(ang, "rotation error deg") <= 1.0
    assert measured(dt, "translation error") <= 0.003
    assert measured(ds, "scale error") <= 0.01
    assert losses[-1] < 0.2 * losses[0]


# ------------------------------------------------------------------ 6. the entry point

def _closed_box_ply(path, lo, hi):
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    lines = ["ply", "format ascii 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
             f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    lines += [" ".join(f"{c:.6f}" for c in p) for p in v] + ["4 " + " ".join(str(i) for i in f) for f in faces]
    Path(path).write_text("\n".join(lines) + "\n")


def _write_regist_experiment(tmp_path, sh_degree=0, num_iter=50):
    from PIL import Image
    from neuma_amd import io as nio, synth
    from neuma_amd.render.gaussian_model import GaussianModel
    W, H = 160, 120
    sc = synth.make_scene("tiny", override=dict(K=3000, W=W, H=H, sh=sh_degree))
    raw = tmp_path / "raw"
    raw.mkdir()
    gm = GaussianModel(sh_degree)
    sh = torch.tensor(sc.g_sh)
    gm.set_params(torch.tensor(sc.g_xyz), sh[:, :1].contiguous(), sh[:, 1:].contiguous(), torch.tensor(sc.g_logscale),
                  torch.tensor(sc.g_rot), torch.tensor(sc.g_opacity_logit))
    nio.save_gaussians_ply(gm, raw / "point_cloud.ply")
    _closed_box_ply(raw / "mesh.ply", (0.35, 0.35, 0.35), (0.65, 0.65, 0.65))
    data = tmp_path / "dataset"
    (data / "data_dynamic").mkdir(parents=True)
    cams = synth.ring_cameras(2, W, H)
    entries = []
    for vi, cam in enumerate(cams):
        c2w = np.linalg.inv(cam.world_view_transform.double().numpy().T)
        c2w[:3, 1:3] *= -1
        fx, fy = nio.fov2focal(cam.FoVx, W), nio.fov2focal(cam.FoVy, H)
        for step in range(2):
            entries.append({"file_path": f"./data_dynamic/r_{vi}_{step:03d}.png", "c2w": c2w[:3].tolist(),
                            "intrinsic": [[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]]})
            img = np.zeros((H, W, 4), np.uint8)
            img[H // 4: 3 * H // 4, W // 3: 2 * W // 3] = 255
            Image.fromarray(img, "RGBA").save(data / entries[-1]["file_path"])
    (data / "data_dynamic.json").write_text(json.dumps(entries))
    cfg = dict(gpu=0, seed=42, debug=True, resume=False, overwrite=False, sim_data_name="regbox", assets_root=str(tmp_path / "assets"),
               gaussian=dict(sh_degree=sh_degree, opacity_thres=0.02, confidence=0.95, max_particles=10,
                             kernels_path=str(raw / "point_cloud.ply")),
               particle_data=dict(mesh_path=str(raw / "mesh.ply"), mesh_sample_mode="volumetric", mesh_sample_resolution=12),
               video_data=dict(eval=False, camera_type="NeuMASynthetic",
                               data=dict(path=str(data), transformsfile="data_dynamic.json", white_background=False, exclude_steps=[-1],
                                         used_views=["r_0", "r_1"], init_frame=0), camera=dict(resolution=1, data_device="cpu")),
               register=dict(views="all", num_iter=num_iter, lr_r=1e-3, lr_t=5e-4, lr_s=1e-4, INIT_R=[2, 0, 0], INIT_T=[0.0, 0.0, 0.0],
                             INIT_S=[1.0], pixel_loss="l1", lambda_ssim_loss=0.1, scheduler=dict(max_steps=num_iter, learning_rate_alpha=0.01)))
    path = tmp_path / "regist-box.yaml"
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))
    return path, cfg


def _run(path):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    return subprocess.run([sys.executable, "-m", "neuma_amd.regist", "-c", str(path)], cwd=str(ROOT), env=env, capture_output=True,
                          text=True, timeout=600)


def test_entry_point_writes_the_registered_assets_and_skips_a_second_time(tmp_path):
    from neuma_amd import io as nio
    from neuma_amd.extras import mesh_sampling as mesh
    from neuma_amd.prepare import prepare_simulation_data
    from neuma_amd.regist import transform_pcd
    path, cfg = _write_regist_experiment(tmp_path)
    p = _run(path)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "Registration finished. Loss:" in p.stdout
    root = tmp_path / "assets" / "regbox"
    z = np.load(root / "registered_params.npz")
    assert sorted(z.files) == ["o", "r", "s", "t"]
    assert z["r"].shape == (3, 3) and z["t"].shape == (3,) and z["s"].shape == (1,) and z["o"].shape == (1, 3)
    assert np.allclose(z["r"] @ z["r"].T, np.eye(3), atol=1e-5)
    g = nio.load_gaussians_ply(root / "registered_kernels.ply", 0)
    assert g._xyz.shape == (3000, 3) and torch.isfinite(g._xyz).all()
    assert torch.allclose(g._rotation.norm(dim=1), torch.ones(3000), atol=1e-5)
    assert (root / "debug" / "regist_iter_1.png").is_file()
    pts = nio.load_particles_ply(root / "registered_particles.ply")
    ref = transform_pcd(mesh.sample_mesh_points(*mesh.read_ply_mesh(tmp_path / "raw" / "mesh.ply"), mode="volumetric", resolution=12),
                        z["s"], z["o"], z["r"], z["t"])
    assert pts.shape == ref.shape and pts.shape[0] > 100
    assert measured(np.abs(pts - ref.astype(np.float32)).max(), "particles vs transform_pcd") <= 1e-6
    stamps = {n: (root / n).stat().st_mtime_ns for n in ("registered_params.npz", "registered_kernels.ply", "registered_particles.ply")}
    p2 = _run(path)
    assert p2.returncode == 0, p2.stdout[-3000:] + p2.stderr[-3000:]
    assert "already finished. Skip." in p2.stdout and p2.stdout.count("Skip.") == 2
    assert stamps == {n: (root / n).stat().st_mtime_ns for n in stamps}
    # the finetune stage's asset preparation accepts the two registered files
    out = tmp_path / "prep"
    prepare_simulation_data(save_dir=out, kernels_path=root / "registered_kernels.ply", particles_path=root / "registered_particles.ply",
                            sh_degree=0, particles_downsample_factor=1, device=dev())
    assert all((out / n).is_file() for n in ("kernels.ply", "particles.ply", "bindings.pt"))


def test_entry_point_rejects_sh_rotation(tmp_path):
    from neuma_amd.config import load_config
    from neuma_amd.regist import regist_gaussians
    path, _ = _write_regist_experiment(tmp_path, sh_degree=1, num_iter=2)
    with pytest.raises(NotImplementedError, match="sh_degree > 0"):
        regist_gaussians(load_config(path))
