"""GPU: constitutive pretraining on particle trajectories (neuma_amd/pretrain.py) on the small body of tests/pretrain_cases.py.

Run-to-run noise as a yardstick: the roll-out's p2g scatter adds with float atomics, so two runs differ in the last bits.  Where a
test compares two ways of computing one quantity it is held to 4 x the difference between two runs of ONE way, the second on a
simulator built with reorder=False (the shuffled particle list is then scattered in another order: different arithmetic for sure,
where two runs in one order may happen to agree bitwise), with a floor of 1e-6 relative (fp32 sums of a few terms)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pretrain_cases as pc
from gpu_util import abs_max, dev, measured, parity

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# tests/test_gpu_rollout.py::test_fused_rollout_equals_per_operator_path_and_oracle: abs_max / max(1, |b|max) of every state tensor
BOUND_FUSED_VS_PER_OPERATOR = 5e-6
# tests/test_gpu_train.py::test_finetune_recovers_...: |l3 - l4| < 5e-3 |l4| + 1e-9 for the fused / per-operator loss of an epoch
BOUND_TRAIN_REL, BOUND_TRAIN_ABS = 5e-3, 1e-9


@pytest.fixture(scope="module")
def case():
    """the body and the two teachers' trajectories, computed once and left unchanged"""
    from neuma_amd.pretrain import generate_trajectory
    model, st, init = pc.body()
    with torch.no_grad():
        jelly = generate_trajectory(model, st, init, *pc.neural_pair("jelly"), pc.T, pc.S)
        coro = generate_trajectory(model, st, init, *pc.corotated(), pc.T, pc.S)
    return dict(model=model, statics=st, init=init, jelly=jelly, corotated=coro)


def stepper(case, E, P, fused="auto", reorder="auto"):
    from neuma_amd.pretrain import FrameStepper
    return FrameStepper(case["model"], case["statics"], E, P, pc.S, pc.T, fused=fused, reorder=reorder)


def weights(E, P):
    return [p for p in list(E.parameters()) + list(P.parameters()) if p.requires_grad]


def flat(ts):
    return torch.cat([t.reshape(-1).double() for t in ts])


# ---------------------------------------------------------------- generator

def test_generator_frames_agree_with_the_fused_rollout(case):
    traj, init = case["jelly"], case["init"]
    assert traj.num_frames == pc.T and traj.meta["substeps"] == pc.S and traj.can_teacher_force
    for rec, t in zip(traj.frame(0), init):
        assert torch.equal(rec, t)                                   # frame 0: the initial state, bitwise
    sim = stepper(case, *pc.neural_pair("jelly"), fused="true")
    state = init
    with torch.no_grad():
        for f in range(1, pc.T + 1):
            state = sim.advance(f - 1, *state)
            for name, a, b in zip("xvCF", traj.frame(f), state):
                err = abs_max(a, b) / max(1.0, float(b.abs().max()))
                parity("pretrain generator vs fused roll-out", f"{name} frame {f}", err, BOUND_FUSED_VS_PER_OPERATOR)


def test_generator_with_a_classical_teacher_stays_finite_and_inside_the_box(case):
    traj = case["corotated"]
    for t in (traj.x, traj.v, traj.C, traj.F):
        assert bool(torch.isfinite(t).all())
    clip = float(traj.meta["clip_bound"])
    assert float(traj.x.min()) >= clip and float(traj.x.max()) <= 1.0 - clip
    assert float((traj.x[-1] - traj.x[0]).abs().max()) > 1e-3                     # it moved
    assert torch.equal(traj.x[0], case["init"][0]) and torch.equal(traj.F[0], case["init"][3])


# ---------------------------------------------------------------- gradient

def epoch_gradient(case, loss_fn, reorder="auto", scale=0.8):
    from neuma_amd.pretrain import epoch_loss
    E, P = pc.neural_pair("jelly", final_scale=scale)
    loss, _ = epoch_loss(stepper(case, E, P, reorder=reorder), case["jelly"], pc.T, loss_fn=loss_fn)
    ws = weights(E, P)
    return float(loss), flat(torch.autograd.grad(loss, ws)), (E, P, ws)


def test_epoch_gradient_native_loss_against_the_torch_composition(case):
    from neuma_amd.state_loss import state_loss, state_loss_torch
    seen = []

    def both(x, v, xg, vg, mask, **kw):          # the two losses on the SAME roll-out outputs, for the value
        seen.append(float(state_loss_torch(x, v, xg, vg, mask, **kw)))
        return state_loss(x, v, xg, vg, mask, **kw)

    l_nat, g_nat, _ = epoch_gradient(case, both)
    l_t1, g_t1, _ = epoch_gradient(case, state_loss_torch)
    l_t2, g_t2, _ = epoch_gradient(case, state_loss_torch, reorder=False)
    assert measured(abs(l_nat - sum(seen)) / l_nat, "epoch loss, native vs torch on the same outputs (rel)") <= 3 * 2.0 ** -22
    gmax = float(g_t1.abs().max())
    noise = float((g_t1 - g_t2).abs().max())
    bound = max(4 * noise, 1e-6 * gmax)
    print(f"PRETRAIN gradient: |g|max {gmax:.3e} run-to-run {noise:.3e} native-vs-torch {float((g_nat - g_t1).abs().max()):.3e}")
    parity("pretrain epoch gradient", "native vs torch loss (abs max)", float((g_nat - g_t1).abs().max()), bound)
    assert gmax > 0 and bool(torch.isfinite(g_nat).all())


# |central difference of the loss along g / |g|^2 - 1|: twice the deviation measured on MI355X (ratio 1.000020)
FD_RATIO_DEV = 4e-5


def test_epoch_gradient_against_the_central_difference_along_itself(case):
    """(L(theta + h g) - L(theta - h g)) / (2 h |g|^2) = 1 for the exact gradient.  h moves the loss by about +-5 %: far above the
    roll-out's run-to-run noise on the loss (~1e-6 relative), small enough for the cubic term."""
    from neuma_amd.pretrain import epoch_loss
    from neuma_amd.state_loss import state_loss
    l0, g, (E, P, ws) = epoch_gradient(case, state_loss)
    g2 = float((g * g).sum())
    h = 0.05 * l0 / g2
    sim = stepper(case, E, P)
    parts, o = [], 0
    for w in ws:
        parts.append(g[o:o + w.numel()].view_as(w).float()); o += w.numel()
    vals = {}
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            for w, d in zip(ws, parts):
                w.add_(sgn * h * d)
            vals[sgn] = float(epoch_loss(sim, case["jelly"], pc.T)[0])
            for w, d in zip(ws, parts):
                w.sub_(sgn * h * d)
    ratio = (vals[1.0] - vals[-1.0]) / (2 * h * g2)
    print(f"PRETRAIN fd: L {l0:.6e} L+ {vals[1.0]:.6e} L- {vals[-1.0]:.6e} h {h:.3e} |g|^2 {g2:.3e} ratio {ratio:.6f}")
    assert vals[1.0] > l0 > vals[-1.0]
    assert measured(abs(ratio - 1.0), "central difference along g over |g|^2, deviation from 1") <= FD_RATIO_DEV


# ---------------------------------------------------------------- teacher forcing

def test_teacher_forcing_cuts_the_epoch_into_independent_frames(case):
    from neuma_amd.pretrain import epoch_loss
    traj = case["jelly"]
    E, P = pc.neural_pair("jelly", final_scale=0.8)
    sim = stepper(case, E, P)
    start = tuple(t.clone().requires_grad_(True) for t in traj.frame(0))
    total, terms = epoch_loss(sim, traj, pc.T, teacher_steps=1, start=start)
    single = [float(epoch_loss(sim, traj.window(f - 1, f), 1)[0]) for f in range(1, pc.T + 1)]
    other = float(epoch_loss(stepper(case, E, P, reorder=False), traj, pc.T, teacher_steps=1)[0])
    noise = abs(float(total) - other)
    bound = max(4 * noise, 1e-6 * float(total))
    print(f"PRETRAIN forcing: epoch {float(total):.6e} sum of frames {sum(single):.6e} run-to-run {noise:.3e}")
    parity("pretrain teacher forcing", "epoch loss vs sum of one-frame losses (abs)", abs(float(total) - sum(single)), bound)
    # frames >= 2 start from recorded states: nothing flows back into frame 0
    late = torch.autograd.grad(sum(terms[1:]), start, retain_graph=True, allow_unused=True)
    assert all(g is None or not bool(g.any()) for g in late)
    first = torch.autograd.grad(terms[0], start[:2], allow_unused=True)
    assert all(g is not None and bool(g.any()) for g in first)
    # without forcing they do
    start2 = tuple(t.clone().requires_grad_(True) for t in traj.frame(0))
    _, free = epoch_loss(sim, traj, pc.T, teacher_steps=0, start=start2)
    assert bool(torch.autograd.grad(sum(free[1:]), start2[0])[0].any())


# ---------------------------------------------------------------- identification: the test with a known answer

# (RAdam: five momentum steps on the clipped gradient, then rectified Adam steps of about 0.05 lr at this epoch count)
IDENT_CFG = dict(num_epochs=30, fused="false", elasticity_lr=0.2, plasticity_lr=0.2,
                 elasticity_scheduler=dict(type="cos", max_steps=30, learning_rate_alpha=0.1),
                 plasticity_scheduler=dict(type="cos", max_steps=30, learning_rate_alpha=0.1))
# final |log_E - log E*|, |sigma_y - sigma_y*| / sigma_y*: twice the residual measured on MI355X
# (log_E: 0.6931 -> 0.1053 in 30 epochs, shrink factor 0.15, loss 3.49 -> 0.048)
IDENT_LOG_E_RESIDUAL = 0.21
# (sigma_y: relative error 0.3333 -> 0.1116 in 30 epochs, loss 0.178 -> 0.0206)
IDENT_SIGMA_Y_RESIDUAL = 0.22


def test_identification_of_log_E_from_a_corotated_trajectory(case):
    from neuma_amd.pretrain import pretrain_constitutive
    E, P = pc.corotated(E=2.0 * pc.E_STAR)
    target = float(np.log(pc.E_STAR))
    start = abs(float(E.log_E) - target)
    losses = pretrain_constitutive(case["model"], case["statics"], case["corotated"], E, P, IDENT_CFG)
    end = abs(float(E.log_E) - target)
    print(f"PRETRAIN identification log_E: |error| {start:.4f} -> {end:.4f} (shrink {end / start:.4f}), loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert len(losses) == 30 and all(np.isfinite(losses))
    assert end < start and losses[-1] < losses[0]
    assert measured(end, "|log_E - log E*| after 30 epochs") <= IDENT_LOG_E_RESIDUAL


def test_identification_of_sigma_y_from_a_von_mises_trajectory(case):
    from neuma_amd.pretrain import generate_trajectory, pretrain_constitutive
    sy = 1.5e4
    e_t, _ = pc.corotated()
    with torch.no_grad():
        traj = generate_trajectory(case["model"], case["statics"], case["init"], e_t, pc.von_mises(sy), pc.T, pc.S)
    assert all(bool(torch.isfinite(t).all()) for t in (traj.x, traj.v, traj.C, traj.F))
    # a row has yielded in the first frame where its F left the purely elastic trajectory of the same elasticity and start
    # (case["corotated"]: IdentityPlasticity); the return map then holds its deviatoric Hencky strain at sigma_y / (2 mu)
    mu = pc.E_STAR / (2 * (1 + pc.NU))
    eps = torch.linalg.svdvals(traj.F[1:].cpu().double()).clamp_min(0.05).log()
    dev_norm = (eps - eps.mean(-1, keepdim=True)).norm(dim=-1)
    yielded = int(((traj.F[1] - case["corotated"].F[1]).abs().amax(dim=(-1, -2)) > 1e-3).sum())
    print(f"PRETRAIN von Mises trajectory: {yielded} rows left the elastic path in frame 1; |dev log sigma| max {float(dev_norm.max()):.4f}, "
          f"yield surface {sy / (2 * mu):.4f}")
    if yielded == 0:
        pytest.skip("no row of the generated trajectory yields: sigma_y cannot be identified from it")
    E, _ = pc.corotated()
    E.log_E.requires_grad_(False)
    P = pc.von_mises(2.0e4)
    P.log_E.requires_grad_(False)                 # only sigma_y is unknown
    start = abs(float(P.sigma_y) - sy) / sy
    losses = pretrain_constitutive(case["model"], case["statics"], traj, E, P, dict(IDENT_CFG, plasticity_lr=5000.0))
    end = abs(float(P.sigma_y) - sy) / sy
    print(f"PRETRAIN identification sigma_y: {yielded} yielding rows, rel error {start:.4f} -> {end:.4f}, loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert all(np.isfinite(losses)) and end < start and losses[-1] < losses[0]
    assert measured(end, "|sigma_y - sigma_y*| / sigma_y* after 30 epochs") <= IDENT_SIGMA_Y_RESIDUAL


# ---------------------------------------------------------------- recovery, checkpoints, resume

NEURAL_CFG = dict(elasticity_lr=3e-2, plasticity_lr=3e-3, ckpt_every=2, num_ckpts=2,
                  elasticity_scheduler=dict(type="cos", max_steps=20, learning_rate_alpha=0.1),
                  plasticity_scheduler=dict(type="cos", max_steps=20, learning_rate_alpha=0.1))


def test_neural_recovery_checkpoints_and_resume(case, tmp_path):
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    from neuma_amd.pretrain import pretrain_constitutive
    model, st, traj = case["model"], case["statics"], case["jelly"]
    E, P = pc.neural_pair("jelly", final_scale=0.8)
    logs = []
    losses = pretrain_constitutive(model, st, traj, E, P, dict(NEURAL_CFG, num_epochs=20, fused="true"), out_root=tmp_path, log=logs.append)
    print(f"PRETRAIN recovery: loss {losses[0]:.4e} -> {losses[-1]:.4e} (ratio {losses[-1] / losses[0]:.4f})")
    assert len(losses) == 20 == len(logs) and all(np.isfinite(losses))
    assert measured(losses[-1] / losses[0], "neural recovery: last loss / first loss") < 1.0
    # the same first 5 epochs through the per-operator path
    E2, P2 = pc.neural_pair("jelly", final_scale=0.8)
    slow = pretrain_constitutive(model, st, traj, E2, P2, dict(NEURAL_CFG, num_epochs=5, fused="false"))
    for a, b in zip(slow, losses[:5]):
        parity("pretrain fused vs per-operator", "epoch loss (abs)", abs(a - b), BOUND_TRAIN_REL * abs(b) + BOUND_TRAIN_ABS)
    # checkpoints: every 2nd epoch and the last, newest two kept
    assert sorted(p.name for p in tmp_path.glob("*.pt")) == ["0018.pt", "0020.pt"]
    pretrained = torch.load(tmp_path / "0020.pt", map_location=dev())
    assert set(pretrained) == {"elasticity", "plasticity", "loss"} and pretrained["loss"] == losses[-1]
    elasticity = InvariantFullMetaElasticity(pc.NET_CFG).to(dev())
    plasticity = InvariantFullMetaPlasticity(pc.NET_CFG).to(dev())
    elasticity.load_state_dict(pretrained["elasticity"])              # finetune.setup's two lines
    plasticity.load_state_dict(pretrained["plasticity"])
    assert all(torch.equal(a, b) for a, b in zip(elasticity.state_dict().values(), E.state_dict().values()))
    # resume: fresh Xavier nets pick the newest checkpoint up and go on from it
    E3, P3 = InvariantFullMetaElasticity(pc.NET_CFG).to(dev()), InvariantFullMetaPlasticity(pc.NET_CFG).to(dev())
    more = pretrain_constitutive(model, st, traj, E3, P3, dict(NEURAL_CFG, num_epochs=1, fused="true", resume=True), out_root=tmp_path)
    assert abs(more[0] - losses[-1]) < 0.5 * losses[-1] + 1e-12
    assert sorted(p.name for p in tmp_path.glob("*.pt")) == ["0020.pt", "0021.pt"]
    # init_ckpt: the same start without the run folder
    E4, P4 = InvariantFullMetaElasticity(pc.NET_CFG).to(dev()), InvariantFullMetaPlasticity(pc.NET_CFG).to(dev())
    again = pretrain_constitutive(model, st, traj, E4, P4, dict(NEURAL_CFG, num_epochs=1, fused="true", init_ckpt=str(tmp_path / "0020.pt")))
    assert abs(again[0] - more[0]) <= BOUND_TRAIN_REL * more[0] + BOUND_TRAIN_ABS


# ---------------------------------------------------------------- entry point

def test_entry_point(tmp_path):
    import yaml
    from neuma_amd import io as nio, pretrain, synth
    nio.save_particles_ply(tmp_path / "ball.ply", synth.ball_particles(pc.N, pc.G))
    unit = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    cfg = dict(seed=0, gpu=0, sim=pc.SIM_CFG, result_root=str(tmp_path / "run"),
               particle_data=dict(particles_path=str(tmp_path / "ball.ply"), vol=(0.5 / pc.G) ** 3, rho=1000.0, clip_bound=0.1,
                                  shape=dict(ori_bounds=unit, sim_bounds=unit), vel=dict(lin_vel=[0.0, -0.5, 0.0], ang_vel=[0.0, 0.0, 3.0])),
               teacher=dict(elasticity=dict(name="CorotatedElasticity", E=pc.E_STAR, nu=pc.NU), plasticity=dict(name="IdentityPlasticity")),
               constitution=dict(elasticity=dict(pc.NET_CFG), plasticity=dict(pc.NET_CFG)),
               pretrain=dict(num_frames=2, substeps=5, num_epochs=2))
    (tmp_path / "tiny.yaml").write_text(yaml.safe_dump(cfg))
    out = tmp_path / "run" / "pretrain"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "neuma_amd.pretrain", "-c", str(tmp_path / "tiny.yaml")],
                       cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(q.name for q in out.glob("*.pt")) == ["0002.pt", "trajectory.pt"]
    from neuma_amd.trajectory import Trajectory
    traj = Trajectory.load(out / "trajectory.pt")
    assert traj.num_frames == 2 and traj.meta["substeps"] == 5 and traj.can_teacher_force
    keys = {k: sorted(v) for k, v in torch.load(out / "0002.pt", map_location="cpu").items() if k != "loss"}
    assert keys["elasticity"] == sorted(("layers.0.fc.weight", "layers.1.fc.weight", "final_layer.fc.weight"))
    # --trajectory: no teacher block needed, the file is reused (in this process: the command line's main)
    cfg2 = {k: v for k, v in cfg.items() if k != "teacher"}
    cfg2["result_root"] = str(tmp_path / "run2")
    (tmp_path / "second.yaml").write_text(yaml.safe_dump(cfg2))
    pretrain.main(["-c", str(tmp_path / "second.yaml"), "--trajectory", str(out / "trajectory.pt")])
    out2 = tmp_path / "run2" / "pretrain"
    assert sorted(q.name for q in out2.glob("*.pt")) == ["0002.pt"]
    assert {k: sorted(v) for k, v in torch.load(out2 / "0002.pt", map_location="cpu").items() if k != "loss"} == keys
    # --generate_only: a trajectory and no checkpoint
    pretrain.main(["-c", str(tmp_path / "tiny.yaml"), "--generate_only", "--result_root", str(tmp_path / "run3")])
    assert sorted(q.name for q in (tmp_path / "run3" / "pretrain").glob("*.pt")) == ["trajectory.pt"]
