"""GPU: constitutive pretraining against unordered point clouds (`loss: chamfer`, neuma_amd/pretrain.py + chamfer_loss.py) on the
small body of tests/pretrain_cases.py.

The yardstick is that of tests/test_gpu_pretrain.py: two ways of computing one gradient are held to 4 x the difference between two
state_loss_torch epochs, the second on a simulator built with reorder=False (the roll-out's float-atomic scatter in another
order), with a floor of 1e-6 |g|max.  That noise is measured on code that does not contain the Chamfer loss.

Bijection identity: when every frame's cloud is the teacher's frame with its rows permuted and the student stays far inside half
the particle spacing, a(i) is the inverse permutation, b(j) the permutation, and with weights (0.5, 0.5) the Chamfer loss is
exactly sum |x - gt|^2 / N = 3 x the l2 position term of state_loss."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pretrain_cases as pc
from gpu_util import dev, measured, parity

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FINAL_SCALE = 0.8                   # the student of tests/test_gpu_pretrain.py: jelly with its final layers scaled
# The bijection identity needs max |x_i - gt_i| < half the smallest distance between two teacher particles: then, by the triangle
# inequality, gt_i is x_i's nearest observation and the other way round.  Measured on MI355X: the teacher's smallest spacing is
# 0.0133 / 0.0109 / 0.0121 in frames 1 / 2 / 3; the student strays by at most 0.0117 at scale 0.8 (one row of frame 3 then
# pairs with a neighbour's observation), 0.0056 at 0.9 (no wrong pair, no margin) and 0.0028 at 0.95 - a quarter of the spacing.
BIJECTION_SCALE = 0.95
RAGGED = (1100, 900, 1300)          # observed rows of frames 1, 2, 3


@pytest.fixture(scope="module")
def case():
    """the body, the teacher's trajectory, the observations made of it and the noise yardstick: computed once, left unchanged"""
    from neuma_amd.pretrain import generate_trajectory
    from neuma_amd.state_loss import state_loss_torch
    from neuma_amd.trajectory import CloudTrajectory, Trajectory
    model, st, init = pc.body()
    with torch.no_grad():
        jelly = generate_trajectory(model, st, init, *pc.neural_pair("jelly"), pc.T, pc.S)
    n = jelly.num_particles
    c = dict(model=model, statics=st, init=init, jelly=jelly, positions=Trajectory(jelly.x, meta=jelly.meta))
    x0, v0, C0, F0 = jelly.frame(0)
    perms = [torch.tensor(np.random.default_rng(100 + f).permutation(n), device=dev()) for f in range(1, pc.T + 1)]
    c["perms"] = perms
    c["permuted"] = CloudTrajectory(x0, [jelly.x[f + 1][p] for f, p in enumerate(perms)], v0, C0, F0, None, jelly.meta)
    subsets = [torch.tensor(np.sort(np.random.default_rng(200 + f).permutation(n)[:m]), device=dev()) for f, m in enumerate(RAGGED)]
    mask = torch.tensor((np.random.default_rng(300).random(n) >= 0.3).astype(np.uint8), device=dev())
    c["ragged"] = CloudTrajectory(x0, [jelly.x[f + 1][s] for f, s in enumerate(subsets)], v0, C0, F0, mask, jelly.meta)
    # the yardstick: two state_loss_torch epochs (positions only), the second on a reorder=False simulator, per student
    c["state"], c["noise"] = {}, {}
    for scale in (FINAL_SCALE, BIJECTION_SCALE):
        l1, g1 = epoch_gradient(c, c["positions"], state_loss_torch, scale=scale)
        l2, g2 = epoch_gradient(c, c["positions"], state_loss_torch, reorder=False, scale=scale)
        c["state"][scale] = (l1, g1)
        c["noise"][scale] = float((g1 - g2).abs().max())
    return c


def stepper(case, E, P, reorder="auto"):
    from neuma_amd.pretrain import FrameStepper
    return FrameStepper(case["model"], case["statics"], E, P, pc.S, pc.T, reorder=reorder)


def epoch_gradient(case, traj, loss_fn, reorder="auto", sim=None, pair=None, scale=FINAL_SCALE):
    from neuma_amd.pretrain import epoch_loss
    E, P = pair or pc.neural_pair("jelly", final_scale=scale)
    sim = sim or stepper(case, E, P, reorder=reorder)
    loss, _ = epoch_loss(sim, traj, pc.T, loss_fn=loss_fn, start=case["init"])
    ws = [p for p in list(E.parameters()) + list(P.parameters()) if p.requires_grad]
    g = torch.cat([t.reshape(-1).double() for t in torch.autograd.grad(loss, ws)])
    return float(loss.detach()), g


def test_bijection_identity_chamfer_is_three_times_the_l2_position_term(case):
    from neuma_amd.chamfer_loss import chamfer_loss, chamfer_loss_raw
    from neuma_amd.state_loss import state_loss
    n = case["jelly"].num_particles
    frames, seen = [], []

    def both(x, v, x_gt, v_gt, mask, **kw):
        f = len(frames)
        perm = case["perms"][f]
        ixy, iyx = torch.empty(n, dtype=torch.int64, device=dev()), torch.empty(n, dtype=torch.int64, device=dev())
        chamfer_loss_raw(x.detach().contiguous(), x_gt, None, 0.5, 0.5, idx_xy=ixy, idx_yx=iyx)
        frames.append(bool(torch.equal(ixy, torch.argsort(perm))) and bool(torch.equal(iyx, perm)))
        seen.append(float(state_loss(x.detach(), None, case["jelly"].x[f + 1], None, None, kind="l2")))      # the same roll-out outputs
        return chamfer_loss(x, x_gt, mask, weight_xy=0.5, weight_yx=0.5)

    l_ch, g_ch = epoch_gradient(case, case["permuted"], both, scale=BIJECTION_SCALE)
    # the precondition, never skipped: every frame's assignment is the permutation and its inverse
    assert len(frames) == pc.T and all(frames), f"final_scale {BIJECTION_SCALE}: the student left its own observation's cell: {frames}"
    assert measured(abs(l_ch - 3.0 * sum(seen)) / l_ch, "epoch loss, chamfer vs 3 x l2 positions on the same outputs (rel)") <= 3 * 2.0 ** -22
    l_st, g_st = case["state"][BIJECTION_SCALE]
    noise = case["noise"][BIJECTION_SCALE]
    gmax = float(g_ch.abs().max())
    bound = max(4 * noise, 1e-6 * gmax)
    diff = float((g_ch - 3.0 * g_st).abs().max())
    print(f"PRETRAIN chamfer bijection: L {l_ch:.6e} 3 L_state {3 * l_st:.6e} |g|max {gmax:.3e} run-to-run {noise:.3e} diff {diff:.3e}")
    parity("pretrain chamfer bijection", "epoch gradient vs 3 x l2 position gradient (abs max)", diff, bound)
    assert gmax > 0 and bool(torch.isfinite(g_ch).all())


def test_ragged_masked_one_sided_epoch_is_finite_and_repeats_within_the_noise(case):
    from neuma_amd.pretrain import chamfer_frame_loss
    fn = chamfer_frame_loss(0.0, 1.0)
    pair = pc.neural_pair("jelly", final_scale=FINAL_SCALE)
    sim = stepper(case, *pair)
    l1, g1 = epoch_gradient(case, case["ragged"], fn, sim=sim, pair=pair)
    l2, g2 = epoch_gradient(case, case["ragged"], fn, sim=sim, pair=pair)
    assert np.isfinite(l1) and l1 > 0 and bool(torch.isfinite(g1).all()) and bool(g1.any())
    gmax = float(g1.abs().max())
    noise = case["noise"][FINAL_SCALE]
    bound = max(4 * noise, 1e-6 * gmax)
    print(f"PRETRAIN chamfer ragged: L {l1:.6e} / {l2:.6e} |g|max {gmax:.3e} run-to-run {float((g1 - g2).abs().max()):.3e} yardstick {noise:.3e}")
    parity("pretrain chamfer ragged", "epoch gradient, two epochs on one simulator (abs max)", float((g1 - g2).abs().max()), bound)


NEURAL_CFG = dict(elasticity_lr=3e-2, plasticity_lr=3e-3,        # test_gpu_pretrain.py::test_neural_recovery_checkpoints_and_resume
                  elasticity_scheduler=dict(type="cos", max_steps=20, learning_rate_alpha=0.1),
                  plasticity_scheduler=dict(type="cos", max_steps=20, learning_rate_alpha=0.1))


def test_descent_on_ragged_observations(case):
    from neuma_amd.pretrain import pretrain_constitutive
    E, P = pc.neural_pair("jelly", final_scale=FINAL_SCALE)
    logs = []
    losses = pretrain_constitutive(case["model"], case["statics"], case["ragged"], E, P,
                                   dict(NEURAL_CFG, num_epochs=20, fused="true", loss="chamfer", weight_xy=1.0, weight_yx=1.0), log=logs.append)
    print(f"PRETRAIN chamfer descent: loss {losses[0]:.4e} -> {losses[-1]:.4e} (ratio {losses[-1] / losses[0]:.4f})")
    assert len(losses) == 20 == len(logs) and all(np.isfinite(losses)) and all("L chamfer" in line for line in logs)
    assert measured(losses[-1] / losses[0], "chamfer descent: last loss / first loss") < 1.0


def test_a_cloud_trajectory_with_another_loss_raises(case):
    from neuma_amd.pretrain import pretrain_constitutive
    from neuma_amd.trajectory import TrajectoryError
    E, P = pc.neural_pair("jelly")
    with pytest.raises(TrajectoryError, match="'loss'"):
        pretrain_constitutive(case["model"], case["statics"], case["ragged"], E, P, dict(loss="l2", num_epochs=1))
    # a plain trajectory may train with the Chamfer loss: its x[f] is the cloud
    losses = pretrain_constitutive(case["model"], case["statics"], case["jelly"], E, P, dict(NEURAL_CFG, loss="chamfer", num_epochs=1))
    assert len(losses) == 1 and np.isfinite(losses[0])


def test_entry_point_on_a_folder_of_ragged_clouds(tmp_path):
    import yaml
    from neuma_amd import io as nio, pretrain, synth
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    from neuma_amd.trajectory import Trajectory
    nio.save_particles_ply(tmp_path / "ball.ply", synth.ball_particles(pc.N, pc.G))
    unit = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    cfg = dict(seed=0, gpu=0, sim=pc.SIM_CFG, result_root=str(tmp_path / "teacher"),
               particle_data=dict(particles_path=str(tmp_path / "ball.ply"), vol=(0.5 / pc.G) ** 3, rho=1000.0, clip_bound=0.1,
                                  shape=dict(ori_bounds=unit, sim_bounds=unit), vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 3.0])),
               teacher=dict(elasticity=dict(name="CorotatedElasticity", E=pc.E_STAR, nu=pc.NU), plasticity=dict(name="IdentityPlasticity")),
               constitution=dict(elasticity=dict(pc.NET_CFG), plasticity=dict(pc.NET_CFG)),
               pretrain=dict(num_frames=2, substeps=5, num_epochs=2, loss="chamfer", weight_xy=1.0, weight_yx=1.0))
    (tmp_path / "teacher.yaml").write_text(yaml.safe_dump(cfg))
    pretrain.main(["-c", str(tmp_path / "teacher.yaml"), "--generate_only"])
    traj = Trajectory.load(tmp_path / "teacher" / "pretrain" / "trajectory.pt")
    scan = tmp_path / "scan"
    scan.mkdir()
    n = traj.num_particles
    for f, m in ((1, n - 300), (2, n - 500)):                                  # ragged: a seeded subset of the teacher's rows per frame
        rows = np.sort(np.random.default_rng(f).permutation(n)[:m])
        nio.save_particles_ply(scan / f"{f:03d}.ply", traj.x[f].numpy()[rows])
    runs = {}
    for kind in ("chamfer", "l2"):
        c2 = {k: v for k, v in cfg.items() if k != "teacher"}
        c2["result_root"] = str(tmp_path / f"run_{kind}")
        c2["pretrain"] = dict(cfg["pretrain"], loss=kind)
        (tmp_path / f"{kind}.yaml").write_text(yaml.safe_dump(c2))
        runs[kind] = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "neuma_amd.pretrain", "-c", str(tmp_path / f"{kind}.yaml"),
                                     "--trajectory", str(scan)], cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True)
    p = runs["chamfer"]
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "L chamfer" in p.stdout
    out = tmp_path / "run_chamfer" / "pretrain"
    assert sorted(q.name for q in out.glob("*.pt")) == ["0002.pt"]
    E, P = InvariantFullMetaElasticity(pc.NET_CFG), InvariantFullMetaPlasticity(pc.NET_CFG)
    ck = pretrain.load_checkpoint(out / "0002.pt", E, P)
    assert np.isfinite(ck["loss"])
    q = runs["l2"]
    assert q.returncode != 0 and "TrajectoryError" in q.stderr and "point-cloud observations are unordered" in q.stderr
    assert not list((tmp_path / "run_l2").glob("**/*.pt"))
