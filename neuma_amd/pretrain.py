"""`python -m neuma_amd.pretrain -c <config.yaml> [--trajectory traj.pt | obs.pt | folder] [--generate_only]` - pretraining of a
constitutive pair on a particle trajectory or on unordered per-frame point clouds: the stage that makes the base model `finetune` and `inference` load through `pretrained_ckpt`.

The reference has NO counterpart: it ships three NCLaw base models (jelly, plasticine, sand) and not their training.  What is
here follows NCLaw's recipe on this project's operators - a teacher material (any of the eight classical laws, or a neural
pair) rolls a body out, the student is fitted to the recorded particle states by BPTT through the simulator:

    generate_trajectory     the per-operator loop  stress = e(F); x, v, C, F = sim(...); F = p(F)  under no_grad, one record
                            every `substeps` substeps, frame 0 = the initial state
    pretrain_constitutive   per epoch: start at frame 0, advance frame by frame, add state_loss(x, v, traj.x[f], traj.v[f]) after
                            every frame (nm_state_loss, state_loss.py), one backward(), clip per module, RAdam steps.
                            A neural pair advances through one MPMFusedDiffSim call per frame (no LoRA: effective_weights() are
                            the plain weights and receive the roll-out's weight gradients); any classical module goes substep by
                            substep through MPMCacheDiffSim - the same loop then identifies log_E / sigma_y / friction_angle.
                            `teacher_steps = k > 0` replaces the running state by the recorded (x, v, C, F) after every k-th frame
                            (NCLaw's teacher forcing; the gradient chain is cut there).
                            Gradients are zeroed every epoch (the never-zeroed quirk of the reference's LoRA loop belongs to
                            train.finetune_constitutive alone).
                            `loss: chamfer` replaces the state loss by chamfer_loss(x, traj.x[f]) (nm_chamfer_loss,
                            chamfer_loss.py): the target of a frame is then an unordered cloud of any size - a CloudTrajectory
                            (trajectory.py: a file with x0 + clouds, or a folder of NNN.ply observations), or a plain Trajectory
                            whose x[f] is taken as the cloud.  Velocities are not compared and there is no teacher forcing.

Config (YAML), the reference's schema where it has one:

    sim: {num_grids, dt, bound, gravity, bc, eps}                     as everywhere
    particle_data: {rho, clip_bound, span?, vel: {lin_vel, ang_vel},  as inference reads them; the cloud comes from
                    shape: {name, asset_root, ori_bounds, sim_bounds, sort?},   <asset_root>/<name>.npz|.ply, or from
                    particles_path?, vol?}                             particles_path (a PLY cloud; vol: per-particle volume,
                                                                       default convex hull / N)
    constitution: {elasticity: {...}, plasticity: {...}}              the student; neural or classical by `name` (material.build)
    teacher: {elasticity, plasticity, pretrained_ckpt?}               the teacher; pretrained_ckpt for a neural one.  Not needed
                                                                       with --trajectory
    pretrain: {...}                                                   PRETRAIN_CFG below (loss: l1 | l2 | chamfer)
    result_root                                                       outputs: <result_root>/pretrain/trajectory.pt, NNNN.pt

Out of scope: the native SceneRuntime.epoch path, sharded / multi-GPU pretraining, classical laws
inside the fused roll-out, several trajectories per epoch, NCLaw's other architectures."""
import argparse
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_
from torch.optim import RAdam

from .material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity, build as build_material
from .chamfer_loss import chamfer_loss
from .state_loss import state_loss
from .train import fetch_scheduler
from .trajectory import CloudTrajectory, Trajectory, TrajectoryError, load_observations, model_meta

RESULT = "results"

PRETRAIN_CFG = dict(
    num_frames=None,            # None: every recorded frame
    substeps=None,              # None: the trajectory's own
    num_epochs=300, teacher_steps=0,
    loss="l2",                  # l1 | l2: state_loss on (x, v) in the simulator's numbering (weight_x, weight_v);
    weight_x=1.0, weight_v=1.0,  # chamfer: chamfer_loss on x against an unordered cloud (weight_xy, weight_yx)
    weight_xy=1.0, weight_yx=1.0,
    fused="auto",               # auto: fused when both modules are neural | true | false
    reorder="auto",             # particle order of the simulators (MPMFusedDiffSim / MPMCacheDiffSim)
    # The learning rates are NOT tuned on any real material (nor on a synthetic one: the recoveries of tests/test_gpu_pretrain.py
    # pass their own, 3e-2 / 3e-3 for a neural pair over 20 epochs, 0.2 for a corotated log_E over 30).  Expect to set them: RAdam
    # takes five plain momentum steps first and rectified steps of a few per cent of lr for the next dozens of epochs.
    elasticity_lr=1e-3, elasticity_wd=0.0, elasticity_grad_max_norm=1.0,
    elasticity_scheduler=dict(type="cos", max_steps=300, learning_rate_alpha=0.05),
    plasticity_lr=1e-4, plasticity_wd=0.0, plasticity_grad_max_norm=1.0,
    plasticity_scheduler=dict(type="cos", max_steps=300, learning_rate_alpha=0.05),
    warmup_step=0, ckpt_every=10, num_ckpts=3, init_ckpt=None, resume=False,
)

_NEURAL = (InvariantFullMetaElasticity, InvariantFullMetaPlasticity)


def is_neural_pair(elasticity, plasticity) -> bool:
    return isinstance(elasticity, InvariantFullMetaElasticity) and isinstance(plasticity, InvariantFullMetaPlasticity)


@torch.no_grad()
def generate_trajectory(model, statics, init_state, elasticity, plasticity, num_frames: int, substeps: int) -> Trajectory:
    """num_frames frames of `substeps` substeps from init_state = (x, v, C, F), the per-operator loop in the order of
    infer.simulate_objects.  The caller's tensors are not touched."""
    from .sim import MPMForwardSim
    x, v, C, F = (t.detach().float().clone().contiguous() for t in init_state)
    frames = [tuple(t.clone() for t in (x, v, C, F))]
    sim = MPMForwardSim(model)
    state = model.state(x.shape[0])
    state.from_torch(x=x, v=v, C=C, F=F, stress=torch.zeros_like(F))
    for _ in range(int(num_frames)):
        for _ in range(int(substeps)):
            state.from_torch(stress=elasticity(F))
            x, v, C, F = sim(statics, state)
            F = plasticity(F)
            state.from_torch(F=F)
        frames.append(tuple(t.clone() for t in (x, v, C, F)))
    meta = dict(model_meta(model), substeps=int(substeps))
    for key in ("rho", "clip_bound"):
        vals = getattr(statics, key)
        if vals.numel() and bool((vals == vals.reshape(-1)[0]).all()):
            meta[key] = float(vals.reshape(-1)[0])
    return Trajectory(*(torch.stack([fr[i] for fr in frames]) for i in range(4)), meta=meta)


class FrameStepper(object):
    """advance(f, x, v, C, F): frame f -> frame f + 1 (`substeps` substeps), differentiable.  fused: one MPMFusedDiffSim node per
    frame (neural pairs only); else MPMCacheDiffSim + the two modules substep by substep."""

    def __init__(self, model, statics, elasticity, plasticity, substeps: int, num_frames: int, fused="auto", reorder="auto") -> None:
        neural = is_neural_pair(elasticity, plasticity)
        if isinstance(fused, str):
            key = fused.lower()
            if key not in ("auto", "true", "false"):
                raise ValueError(f"fused must be auto, true or false, not {fused!r}")
            fused = neural if key == "auto" else key == "true"
        if fused and not neural:
            raise ValueError("fused: true needs a neural pair (InvariantFullMetaElasticity + InvariantFullMetaPlasticity): classical "
                             "laws are not in the fused roll-out")
        self.fused, self.S = bool(fused), int(substeps)
        self.statics, self.elasticity, self.plasticity = statics, elasticity, plasticity
        if self.fused:
            from .rollout import MPMFusedDiffSim
            self.sim = MPMFusedDiffSim(model, elasticity, plasticity, self.S, reorder=reorder)
        else:
            from .sim import MPMCacheDiffSim
            self.sim = MPMCacheDiffSim(model, self.S * int(num_frames), reorder=reorder)

    def advance(self, f: int, x, v, C, F):
        if self.fused:
            return self.sim(self.statics, x, v, C, F)
        for s in range(self.S):
            stress = self.elasticity(F)
            x, v, C, F = self.sim(self.statics, f * self.S + s, x, v, C, F, stress)
            F = self.plasticity(F)
        return x, v, C, F


def epoch_loss(stepper: FrameStepper, traj: Trajectory, num_frames: int, teacher_steps: int = 0, kind: str = "l2",
               weight_x: float = 1.0, weight_v: float = 1.0, loss_fn=state_loss, start=None):
    """One epoch's forward pass: (sum of the frame terms, [term of frame 1, ..., term of frame num_frames]).  start: the
    (x, v, C, F) to begin from instead of the trajectory's frame 0 (it may require gradients)."""
    k = int(teacher_steps)
    if k > 0:
        traj.forcing_state(0)                 # raises when C / F were not recorded
    if start is None:
        x0, v0, C0, F0 = traj.frame(0)
        n = traj.num_particles
        eye = torch.eye(3, dtype=torch.float32, device=x0.device)
        start = (x0, v0 if v0 is not None else torch.zeros_like(x0), C0 if C0 is not None else torch.zeros(n, 3, 3, device=x0.device),
                 F0 if F0 is not None else eye.repeat(n, 1, 1))
    x, v, C, F = start
    terms = []
    for f in range(1, int(num_frames) + 1):
        x, v, C, F = stepper.advance(f - 1, x, v, C, F)
        terms.append(loss_fn(x, v, traj.x[f], None if traj.v is None else traj.v[f], traj.mask, kind=kind, weight_x=weight_x,
                             weight_v=weight_v))
        if k > 0 and f % k == 0 and f < num_frames:
            x, v, C, F = traj.forcing_state(f)
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    return total, terms


def chamfer_frame_loss(weight_xy: float = 1.0, weight_yx: float = 1.0, loss=chamfer_loss):
    """chamfer_loss under epoch_loss's loss_fn signature: x against the frame's cloud x_gt; v, v_gt and the state loss's kind and
    weights are ignored."""
    def fn(x, v, x_gt, v_gt, mask, kind=None, weight_x=None, weight_v=None):
        return loss(x, x_gt, mask, weight_xy=weight_xy, weight_yx=weight_yx)
    return fn


def check_loss_kind(traj, cfg: Dict) -> bool:
    """Whether the configuration asks for the Chamfer loss; raises, naming the key, where the loss and the observations do not go
    together.  traj: the observations, or True for point clouds that are not loaded yet."""
    kind = cfg["loss"]
    if kind not in ("l1", "l2", "chamfer"):
        raise ValueError(f"pretrain 'loss' must be l1, l2 or chamfer, not {kind!r}")
    clouds = traj is True or isinstance(traj, CloudTrajectory)
    if clouds and kind != "chamfer":
        raise TrajectoryError(f"point-cloud observations are unordered: 'loss' = {kind!r} compares rows one to one, only "
                              f"'loss: chamfer' can train on them")
    if clouds and int(cfg["teacher_steps"]) > 0:
        raise TrajectoryError(f"'teacher_steps' = {cfg['teacher_steps']}: point-cloud observations hold no state to restart from")
    return kind == "chamfer"


def checkpoints(root: Path) -> List[Path]:
    """NNNN.pt files of a run, oldest first by epoch number"""
    return sorted((p for p in Path(root).glob("*.pt") if re.fullmatch(r"\d{4,}", p.stem)), key=lambda p: int(p.stem))


def save_checkpoint(path, elasticity, plasticity, loss: float) -> None:
    """{'elasticity', 'plasticity', 'loss'}: for a neural pair the key names of the shipped base models, so the file loads
    through `pretrained_ckpt` unchanged."""
    def sd(m):
        return {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    torch.save({"elasticity": sd(elasticity), "plasticity": sd(plasticity), "loss": float(loss)}, path)


def load_checkpoint(path, elasticity, plasticity, device=None) -> dict:
    ck = torch.load(path, map_location=device if device is not None else "cpu")
    elasticity.load_state_dict(ck["elasticity"])
    plasticity.load_state_dict(ck["plasticity"])
    return ck


def pretrain_constitutive(model, statics, traj, elasticity, plasticity, cfg: Optional[Dict] = None, out_root=None,
                          log=None, loss_fn=None) -> List[float]:
    """Fit (elasticity, plasticity) to the trajectory (a Trajectory, or a CloudTrajectory with `loss: chamfer`); returns the
    per-epoch losses.  cfg: PRETRAIN_CFG keys.  loss_fn: None = state_loss, or the Chamfer adaptor with `loss: chamfer`.  With
    `resume` the newest NNNN.pt of out_root is loaded and the epochs are numbered on from it (the schedules start afresh)."""
    c = dict(PRETRAIN_CFG)
    c.update(cfg or {})
    chamfer = check_loss_kind(traj, c)
    if loss_fn is None:
        loss_fn = chamfer_frame_loss(float(c["weight_xy"]), float(c["weight_yx"])) if chamfer else state_loss
    device = model.device
    S = int(c["substeps"] if c["substeps"] is not None else traj.meta.get("substeps", 0))
    if S <= 0:
        raise TrajectoryError("substeps per frame: neither in the configuration nor in the trajectory's meta")
    nframes = int(c["num_frames"] if c["num_frames"] is not None else traj.num_frames)
    if not 1 <= nframes <= traj.num_frames:
        raise TrajectoryError(f"num_frames = {nframes}, the trajectory has {traj.num_frames} frames after the initial one")
    traj.check_against(model, substeps=S, statics=statics)
    traj = traj.to(device)
    if int(c["teacher_steps"]) > 0:
        traj.forcing_state(0)
    stepper = FrameStepper(model, statics, elasticity, plasticity, S, nframes, fused=c["fused"], reorder=c["reorder"])
    first = 0
    if out_root is not None:
        out_root = Path(out_root)
        out_root.mkdir(parents=True, exist_ok=True)
    if c["init_ckpt"] is not None:
        load_checkpoint(c["init_ckpt"], elasticity, plasticity, device)
    if out_root is not None and c["resume"]:
        prev = checkpoints(out_root)
        if prev:
            load_checkpoint(prev[-1], elasticity, plasticity, device)
            first = int(prev[-1].stem)
    opts = []                                   # (module, optimiser, scheduler, lr, max_norm, params)
    for tag, m in (("elasticity", elasticity), ("plasticity", plasticity)):
        params = [p for p in m.parameters() if p.requires_grad]
        if not params:                          # IdentityPlasticity, SigmaPlasticity: nothing to fit
            continue
        opt = RAdam(params, lr=c[f"{tag}_lr"], weight_decay=c[f"{tag}_wd"])
        opts.append((tag, opt, fetch_scheduler(c[f"{tag}_scheduler"]).get_scheduler(opt, c[f"{tag}_lr"]), c[f"{tag}_lr"],
                     c[f"{tag}_grad_max_norm"], params))
    if not opts:
        raise ValueError("neither module has a trainable parameter")
    losses = []
    last = first + int(c["num_epochs"])
    for epoch in range(first + 1, last + 1):
        step = epoch - first
        if c["warmup_step"] != 0 and step <= c["warmup_step"]:
            for _, opt, _, lr, _, _ in opts:
                for g in opt.param_groups:
                    g["lr"] = lr * float(step) / c["warmup_step"]
        for _, opt, _, _, _, _ in opts:
            opt.zero_grad(set_to_none=True)
        loss, _ = epoch_loss(stepper, traj, nframes, c["teacher_steps"], c["loss"], c["weight_x"], c["weight_v"], loss_fn)
        loss.backward()
        norms = {}
        for tag, opt, _, _, max_norm, params in opts:
            norms[tag] = float(clip_grad_norm_(params, max_norm=max_norm, error_if_nonfinite=True))
            opt.step()
        losses.append(float(loss))
        if log is not None:
            log(f"[Epoch {epoch}/{last} | L {'chamfer' if chamfer else 'state'}: {losses[-1]:.4e} | " +
                " | ".join(f"{tag[0]}-lr: {opt.param_groups[0]['lr']:.2e} | {tag[0]}-gd: {norms[tag]:.2e}" for tag, opt, *_ in opts) + "]")
        if out_root is not None and (step % int(c["ckpt_every"]) == 0 or epoch == last):
            save_checkpoint(out_root / f"{epoch:04d}.pt", elasticity, plasticity, losses[-1])
            files = checkpoints(out_root)
            for old in files[:max(len(files) - int(c["num_ckpts"]), 0)]:
                old.unlink()
        if c["warmup_step"] == 0 or step > c["warmup_step"]:
            for _, _, sch, _, _, _ in opts:
                sch.step()
    return losses


# ---------------------------------------------------------------- entry point

def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", "-c", type=str, required=True, help="Path to the config file.")
    p.add_argument("--trajectory", type=str, default=None,
                   help="Train on these observations instead of generating a trajectory: a trajectory file, a point-cloud "
                        "observation file, or a folder of NNN.ply clouds (loss: chamfer).")
    p.add_argument("--generate_only", action="store_true", help="Write the teacher's trajectory and stop.")
    p.add_argument("--result_root", type=str, default=None)
    return p.parse_args(argv)


def _build_pair(block, device, ckpt=None):
    e = build_material(block.elasticity, InvariantFullMetaElasticity).to(device)
    p = build_material(block.plasticity, InvariantFullMetaPlasticity).to(device)
    nets = [(k, m) for k, m in (("elasticity", e), ("plasticity", p)) if isinstance(m, _NEURAL)]
    if nets and ckpt is not None:
        ck = torch.load(ckpt, map_location=device)
        for k, m in nets:
            m.load_state_dict(ck[k])
    return e, p


def _init_data(pd, total_steps: int):
    from . import io as nio
    from .sim import MPMInitData
    if pd.get("span") is None:
        pd.span = [0, total_steps + 1]
    if pd.get("particles_path") is not None:
        pts = nio.load_particles_ply(Path(pd.particles_path))
        vol = pd.get("vol")
        if vol is None:
            from scipy.spatial import ConvexHull
            vol = float(ConvexHull(pts).volume) / pts.shape[0]
        body = MPMInitData.from_points(pts, float(vol), pd.shape.ori_bounds, pd.shape.sim_bounds, pd.shape.get("sort"))
        data = MPMInitData(rho=pd.rho, clip_bound=pd.clip_bound, span=tuple(pd.span), **body)
    else:
        data = MPMInitData.get(pd)
    if pd.get("vel") is not None:
        data.set_lin_vel(np.array(pd.vel.lin_vel, dtype=np.float64))
        data.set_ang_vel(np.array(pd.vel.ang_vel, dtype=np.float64))
    return data


def pretrain(cfg, trajectory=None, generate_only: bool = False, log=print):
    """The entry point's body.  Returns (trajectory path, per-epoch losses)."""
    from .sim import MPMModelBuilder, MPMStateInitializer, MPMStaticsInitializer
    from .sim.colliders import refuse_in_training
    refuse_in_training(cfg, "python -m neuma_amd.pretrain")
    pc = dict(cfg.get("pretrain") or {})
    # the observations first: what does not go together raises before any device work
    folder = trajectory is not None and Path(trajectory).is_dir()
    if folder:                  # NNN.ply point clouds; their start state is particle_data's (below)
        check_loss_kind(True, dict(PRETRAIN_CFG, **pc))
        frames = [int(p.stem) for p in Path(trajectory).glob("*.ply") if p.stem.isdigit()]
        if not frames or max(frames) < 1:
            raise TrajectoryError(f"no NNN.ply observation after frame 0 in {trajectory}")
        T, S = int(pc.get("num_frames") or max(frames)), int(pc.get("substeps") or 0)
        if S <= 0:
            raise TrajectoryError("'substeps' per frame must be in the configuration: a folder of clouds has no meta")
    elif trajectory is not None:
        traj = load_observations(trajectory)
        check_loss_kind(traj, dict(PRETRAIN_CFG, **pc))
        T = int(pc.get("num_frames") or traj.num_frames)
        S = int(pc.get("substeps") or traj.meta.get("substeps", 0))
    else:
        T, S = int(pc["num_frames"]), int(pc["substeps"])
    seed = int(cfg.get("seed", 0))
    np.random.seed(seed); torch.manual_seed(seed)
    device = torch.device(f"cuda:{cfg.get('gpu', 0)}")
    torch.cuda.set_device(device)
    out_root = Path(cfg.get("result_root") or RESULT) / "pretrain"
    out_root.mkdir(parents=True, exist_ok=True)
    model = MPMModelBuilder().parse_cfg(cfg.sim).finalize(device, requires_grad=True)
    data = _init_data(cfg.particle_data, T * S)
    state_init, statics_init = MPMStateInitializer(model), MPMStaticsInitializer(model)
    state_init.add_group(data); statics_init.add_group(data)
    state, _ = state_init.finalize()
    statics = statics_init.finalize()
    traj_path = out_root / "trajectory.pt"
    if trajectory is None:
        te, tp = _build_pair(cfg.teacher, device, cfg.teacher.get("pretrained_ckpt"))
        traj = generate_trajectory(model, statics, state.to_torch()[:4], te.eval(), tp.eval(), T, S)
        traj.save(traj_path)
        log(f"Wrote {traj_path}: {T} frames of {S} substeps, {traj.num_particles} particles")
    else:
        traj_path = Path(trajectory)
        start = tuple(t.detach().float().cpu() for t in state.to_torch()[:4])
        if folder:
            traj = load_observations(trajectory, **dict(zip(("x0", "v0", "C0", "F0"), start)))
        if traj.num_particles != state.particle.x.shape[0]:
            raise TrajectoryError(f"{trajectory} has {traj.num_particles} particles, particle_data gives {state.particle.x.shape[0]}")
        if isinstance(traj, CloudTrajectory):       # what the observations do not say about the start is particle_data's
            for key, t in zip(("v0", "C0", "F0"), start[1:]):
                if getattr(traj, key) is None:
                    setattr(traj, key, t)
    if generate_only:
        return traj_path, []
    e, p = _build_pair(cfg.constitution, device)
    losses = pretrain_constitutive(model, statics, traj, e, p, dict(pc, num_frames=T, substeps=S), out_root=out_root, log=log)
    return traj_path, losses


def main(argv=None):
    from .config import load_config
    args = parse_args(argv)
    cfg = load_config(args.config)
    if args.result_root is not None:
        cfg["result_root"] = args.result_root
    pretrain(cfg, trajectory=args.trajectory, generate_only=args.generate_only)


if __name__ == "__main__":
    sys.exit(main())
