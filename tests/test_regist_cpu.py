"""CPU: Gaussian registration (neuma_amd.regist, experiments/regist.py) - the four shipped regist-*.yaml parse into the expected
register settings, the pytorch3d-convention rotation conversions hold their identities and hand-computed values (parity with
pytorch3d itself is unpinned: DESIGN §2), transform_pcd and the cosine schedule agree with the reference-generated fixture, and
the ctypes table covers the new entry points."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
INPUTS_DIGEST = "7991c0ea10ad858d"      # sha256 (first 16 hex) of every array regist_inputs rebuilds


@pytest.mark.parametrize("obj", ["bun", "burger", "dog", "pig"])
def test_shipped_regist_configs_parse(obj):
    from neuma_amd.config import load_config
    cfg = load_config(GOLD / "regist_configs" / f"regist-{obj}.yaml")
    rc = cfg.register
    assert rc.num_iter == 20000 and rc.scheduler.max_steps == 20000 and rc.scheduler.learning_rate_alpha == 0.01
    assert (rc.lr_r, rc.lr_t, rc.lr_s) == (1e-4, 5e-5, 1e-5)
    assert len(rc.INIT_R) == 3 and len(rc.INIT_T) == 3 and len(rc.INIT_S) == 1
    assert rc.get("views", "all") == "all" and rc.get("pixel_loss", "l1") == "l1"
    assert cfg.video_data.camera_type == "RealCapture" and cfg.sim_data_name == f"real-{obj}"
    assert cfg.gaussian.sh_degree == 0 and cfg.particle_data.mesh_sample_mode == "volumetric"
    lam = float(rc.get("lambda_ssim_loss", 0.0))
    mask = bool(cfg.video_data.data.get("read_mask_only", False))
    mod = cfg.gaussian.get("scaling_modifier", 1.0)
    assert (lam, mask) == ((0.1, True) if obj == "pig" else (0.0, False))
    assert mod == (1.2 if obj == "dog" else 1.0)


def test_register_initial_values_follow_the_config():
    from neuma_amd.config import load_config
    from neuma_amd.regist import Register, rot6d_to_rotmat, euler_to_rotmat
    rc = load_config(GOLD / "regist_configs" / "regist-burger.yaml").register
    reg = Register(rc, device="cpu")
    reg.training_setup()
    assert reg.r.shape == (6,) and reg.t.tolist() == pytest.approx([0.12, 0.29, -0.21]) and reg.s.tolist() == pytest.approx([0.15])
    assert torch.allclose(reg.get_rotmat, euler_to_rotmat(torch.tensor([60.0, 0.0, 0.0]) * math.pi / 180), atol=1e-6)
    assert torch.allclose(reg.get_euler, torch.tensor([60.0, 0.0, 0.0]), atol=1e-4)
    assert [g["lr"] for g in reg.optimizer.param_groups] == pytest.approx([1e-4, 5e-5, 1e-5])
    assert reg.optimizer.defaults["eps"] == 1e-15 and isinstance(reg.optimizer, torch.optim.RAdam)


def test_euler_to_quat_hand_value():
    from neuma_amd.regist import euler_to_quat
    q = euler_to_quat(torch.tensor([60.0, 0.0, 0.0], dtype=torch.float64) * math.pi / 180)
    assert torch.allclose(q, torch.tensor([math.cos(math.radians(30)), math.sin(math.radians(30)), 0.0, 0.0], dtype=torch.float64), atol=1e-12)
    q = euler_to_quat(torch.tensor([0.0, 90.0, 0.0], dtype=torch.float64) * math.pi / 180)
    assert torch.allclose(q, torch.tensor([math.sqrt(0.5), 0.0, math.sqrt(0.5), 0.0], dtype=torch.float64), atol=1e-12)


def test_rotation_round_trips_and_every_quaternion_branch():
    from neuma_amd import regist as R
    g = torch.Generator().manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(4000, 4, generator=g, dtype=torch.float64), dim=-1)
    q = torch.where(q[:, :1] < 0, -q, q)
    m = R.quat_to_rotmat(q)
    assert torch.allclose(m @ m.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand(4000, 3, 3), atol=1e-12)
    assert torch.allclose(R.rotmat_to_quat(m), q, atol=1e-12)
    assert torch.allclose(R.rot6d_to_rotmat(R.rotmat_to_rot6d(m)), m, atol=1e-12)
    assert torch.allclose(R.rot6d_to_quat(R.quat_to_rot6d(q)), q, atol=1e-12)
    # the four candidates of matrix_to_quaternion: 1 + m00 + m11 + m22, 1 + m00 - m11 - m22, ... largest
    d = torch.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                     1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], -1)
    assert sorted(set(d.argmax(-1).tolist())) == [0, 1, 2, 3]
    # one rotation of pi about each axis: branches 1..3 in isolation, w = 0 (then the sign is the candidate's own)
    for axis, branch in ((0, 1), (1, 2), (2, 3)):
        e = torch.zeros(3, dtype=torch.float64)
        e[axis] = math.pi
        qq = R.euler_to_quat(e)
        want = torch.zeros(4, dtype=torch.float64)
        want[branch] = 1.0
        assert torch.allclose(qq.abs(), want, atol=1e-12)
    # Euler XYZ round trip inside the principal range
    e = (torch.rand(500, 3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([6.0, 3.0, 6.0], dtype=torch.float64)
    assert torch.allclose(R.quat_to_euler(R.euler_to_quat(e)), e, atol=1e-10)
    # 6D: Gram-Schmidt, rows, proper rotation
    d6 = torch.randn(200, 6, generator=g, dtype=torch.float64)
    M = R.rot6d_to_rotmat(d6)
    assert torch.allclose(M[:, 0], torch.nn.functional.normalize(d6[:, :3], dim=-1), atol=1e-12)
    assert torch.allclose(torch.det(M), torch.ones(200, dtype=torch.float64), atol=1e-12)


def test_conversions_agree_with_the_fixture_standin_and_are_differentiable():
    import sys
    sys.path.insert(0, str(GOLD))
    import pytorch3d_transforms as p3d
    from neuma_amd import regist as R
    g = torch.Generator().manual_seed(1)
    d6 = torch.randn(300, 6, generator=g, dtype=torch.float64)
    m = R.rot6d_to_rotmat(d6)
    assert torch.allclose(m, p3d.rotation_6d_to_matrix(d6), atol=1e-14)
    assert torch.allclose(R.rotmat_to_quat(m), p3d.matrix_to_quaternion(m), atol=1e-14)
    e = torch.randn(300, 3, generator=g, dtype=torch.float64)
    assert torch.allclose(R.euler_to_rotmat(e), p3d.euler_angles_to_matrix(e, "XYZ"), atol=1e-14)
    r = d6[0].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: R.rot6d_to_quat(x), (r,))


def test_register_forward_matches_the_fixture():
    """Register.forward (torch path) against the reference's chain at the fixture's R / q_R (R and q_R of the fixture are
    consistent: q_R = matrix_to_quaternion(R))."""
    from neuma_amd import regist as R
    from neuma_amd.render import build_cov3D
    import sys
    sys.path.insert(0, str(GOLD))
    import regist_inputs as ri
    z = np.load(GOLD / "regist" / "regist_transform.npz")
    inp = {k: torch.tensor(v, dtype=torch.float64) for k, v in ri.transform_inputs().items()}
    rows = slice(0, None, ri.ROW_STRIDE)
    for c in ("c0", "c1"):
        g = lambda k: torch.tensor(z[f"{c}_{k}"], dtype=torch.float64)
        Rm, q = g("R"), g("q_R")
        assert torch.allclose(R.rotmat_to_quat(Rm), q, atol=1e-6)
        o = inp["xyz"].mean(0, keepdim=True)
        assert torch.allclose(o, g("o"), atol=1e-15)
        pts = (g("s") * (inp["xyz"] - o)) @ Rm.T + g("t")[None]
        ls = inp["log_scales"] + torch.log(g("s"))
        rot = torch.nn.functional.normalize(R.quaternion_multiply(torch.nn.functional.normalize(inp["rot"], dim=-1), q[None]), dim=-1)
        cov = build_cov3D(torch.exp(ls), rot, float(z[f"{c}_scaling_modifier"][0]))
        assert torch.allclose(pts[rows], g("means3D"), atol=1e-12)
        assert torch.allclose(rot[rows], g("out_rot"), atol=1e-12)
        assert torch.allclose(cov[rows], g("cov6"), rtol=1e-10, atol=1e-14)


def test_transform_pcd_and_schedule_match_the_fixture():
    from neuma_amd.regist import Register, transform_pcd
    import sys
    sys.path.insert(0, str(GOLD))
    import regist_inputs as ri
    z = np.load(GOLD / "regist" / "regist_transform.npz")
    out = transform_pcd(ri.pcd_points(), z["c1_s"].astype(np.float64), z["c1_o"], z["c1_R"], z["c1_t"].astype(np.float64))
    assert np.allclose(out, z["pcd_out"], rtol=0, atol=1e-15)
    cfg = dict(INIT_R=[0, 0, 0], INIT_T=[0, 0, 0], INIT_S=[1.0], lr_r=1e-4, lr_t=5e-5, lr_s=1e-5,
               scheduler=dict(max_steps=20000, learning_rate_alpha=0.01))
    reg = Register(cfg, device="cpu")
    reg.training_setup()
    got = []
    steps = z["sched_steps"].tolist()
    for step in range(20001):
        if step in steps:
            got.append([g["lr"] for g in reg.optimizer.param_groups])
        reg.scheduler.step()
    assert np.allclose(np.array(got), z["sched_lr"], rtol=1e-12, atol=0)


def test_ema_is_the_reference_formula():
    from neuma_amd.regist import ema_of
    hist = [0.5, 0.25, 0.125, 1.0]
    ema = 0.0
    for v in hist:
        ema = 0.4 * v + 0.6 * ema
    assert ema_of(hist) == ema


def test_fixture_inputs_are_rebuilt_exactly():
    """the fixtures store no inputs: regist_inputs rebuilds them from an integer hash with exact arithmetic; pin a few bits so
    that a change of the recipe cannot pass unnoticed (the stored outputs would no longer belong to the inputs)"""
    import hashlib
    import sys
    sys.path.insert(0, str(GOLD))
    import regist_inputs as ri
    inp = ri.transform_inputs()
    assert inp["xyz"].shape == (4096, 3) and all(v.dtype == np.float32 for v in inp.values())
    assert np.abs(np.sqrt((inp["rot"].astype(np.float64) ** 2).sum(1)) - 1).max() > 0.5            # not normalised
    assert inp["log_scales"][:512].min() >= 0.5 and inp["log_scales"][512:1024].max() <= -9.0
    h = hashlib.sha256()
    for k in sorted(inp):
        h.update(inp[k].tobytes())
    for hw in ri.SSIM_SIZES:
        for a in ri.ssim_images(*hw):
            assert a.min() >= 0 and a.max() <= 1
            h.update(a.tobytes())
    h.update(ri.pcd_points().tobytes())
    assert h.hexdigest()[:16] == INPUTS_DIGEST


def test_ctypes_table_covers_the_registration_entry_points():
    from neuma_amd import _lib
    for name in ("nm_regist_apply", "nm_regist_backward", "nm_regist_bwd_workspace", "nm_ssim_loss", "nm_ssim_workspace"):
        assert name in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.nm_regist_bwd_workspace(200000) == 512 * 17 * 8
    assert lib.nm_regist_bwd_workspace(100) == 17 * 8
    assert lib.nm_ssim_workspace(1080, 1920) >= 9 * 1080 * 1920 * 4
    assert lib.nm_ssim_workspace(0, 10) == 0
    # argument checks run before any device work
    assert lib.nm_ssim_loss(1.0, 0, 10, None, None, None, None, None, 0, None) == -1
    assert lib.nm_regist_apply(-1, None, None, None, None, 1.0, None, None, None, None, None) == -1


def test_public_ssim_and_entry_point_are_exposed():
    from neuma_amd import tune
    from neuma_amd.regist import main, parse_args
    assert callable(tune.ssim) and callable(main)
    assert parse_args(["-c", "x.yaml"]).config == "x.yaml"
    with pytest.raises(NotImplementedError):
        tune.ssim(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), window_size=7)
