"""Recorded particle trajectories: the targets of constitutive pretraining (pretrain.py).

A Trajectory holds T + 1 frames of N particles, frame 0 being the initial state:

    x (T+1, N, 3)            positions                          required
    v (T+1, N, 3)            velocities                         optional (without it the supervision is position-only)
    C, F (T+1, N, 3, 3)      affine momentum, deformation       optional, only together (needed for teacher forcing)
    mask (N)                 rows the loss keeps                optional
    meta                     the simulator the frames came from: MODEL_KEYS (what MPMModelBuilder.parse_cfg consumes) plus
                             substeps per frame, and rho / clip_bound of the particles

On disk it is one torch.save dict of CPU fp32 tensors (mask: uint8) and plain-Python meta.  The reference has no counterpart.

A CloudTrajectory holds what comes from outside the simulator instead: the initial state and one unordered point cloud per frame,
of any size (the targets of `loss: chamfer`).  load_observations(path) returns whichever kind the file or folder holds."""
from pathlib import Path
from typing import Optional

import numpy as np
import torch
from torch import Tensor

MODEL_KEYS = ("num_grids", "dt", "bound", "gravity", "bc", "eps")       # MPMModelBuilder.parse_cfg
META_KEYS = MODEL_KEYS + ("substeps", "rho", "clip_bound")


class TrajectoryError(ValueError):
    pass


def _plain(v):
    if isinstance(v, (np.ndarray, Tensor)):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(a) for a in v]
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


def model_meta(model) -> dict:
    """The MODEL_KEYS of a built MPMModel."""
    c = model.constant
    return dict(num_grids=int(c.num_grids), dt=float(c.dt), bound=int(c.bound), gravity=[float(g) for g in np.asarray(c.gravity).reshape(3)],
                bc=str(model.bc), eps=float(c.eps))


class Trajectory(object):

    def __init__(self, x: Tensor, v: Optional[Tensor] = None, C: Optional[Tensor] = None, F: Optional[Tensor] = None,
                 mask: Optional[Tensor] = None, meta: Optional[dict] = None) -> None:
        self.x, self.v, self.C, self.F, self.mask = x, v, C, F, mask
        self.meta = {k: _plain(val) for k, val in dict(meta or {}).items()}
        self.validate()

    # -- shape
    @property
    def num_frames(self) -> int:
        """T: frames after the initial one"""
        return int(self.x.shape[0]) - 1

    @property
    def num_particles(self) -> int:
        return int(self.x.shape[1])

    @property
    def can_teacher_force(self) -> bool:
        return self.v is not None and self.C is not None and self.F is not None

    def validate(self) -> None:
        x = self.x
        if not isinstance(x, Tensor) or x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1:
            raise TrajectoryError(f"x must be (T+1, N, 3), got {tuple(getattr(x, 'shape', ()))}")
        t1, n = int(x.shape[0]), int(x.shape[1])
        for name, want in (("v", (t1, n, 3)), ("C", (t1, n, 3, 3)), ("F", (t1, n, 3, 3)), ("mask", (n,))):
            t = getattr(self, name)
            if t is not None and tuple(t.shape) != want:
                raise TrajectoryError(f"{name} has shape {tuple(t.shape)}, but x {tuple(x.shape)} asks for {want}")
        if (self.C is None) != (self.F is None):
            raise TrajectoryError("C and F are recorded together or not at all")

    # -- access
    def to(self, device) -> 'Trajectory':
        mv = lambda t: None if t is None else t.to(device)      # noqa: E731
        return Trajectory(mv(self.x), mv(self.v), mv(self.C), mv(self.F), mv(self.mask), self.meta)

    def window(self, first: int, last: int) -> 'Trajectory':
        """Frames first..last (inclusive) as a trajectory of their own (views, nothing is copied): `first` becomes frame 0."""
        if not 0 <= first <= last <= self.num_frames:
            raise TrajectoryError(f"window [{first}, {last}] outside frames 0..{self.num_frames}")
        cut = lambda t: None if t is None else t[first:last + 1]        # noqa: E731
        return Trajectory(cut(self.x), cut(self.v), cut(self.C), cut(self.F), self.mask, self.meta)

    def frame(self, f: int):
        """(x, v, C, F) of frame f, None for what was not recorded"""
        return tuple(None if t is None else t[f] for t in (self.x, self.v, self.C, self.F))

    def forcing_state(self, f: int):
        """The detached (x, v, C, F) of frame f to restart a roll-out from (teacher forcing)."""
        if not self.can_teacher_force:
            missing = [k for k in ("v", "C", "F") if getattr(self, k) is None]
            raise TrajectoryError(f"teacher forcing needs the full state of every frame; this trajectory has no {', '.join(missing)}")
        return tuple(t[f].detach().clone() for t in (self.x, self.v, self.C, self.F))

    def check_against(self, model, substeps: Optional[int] = None, statics=None) -> None:
        """Raise, naming the key, when meta disagrees with the simulator about to train on the trajectory."""
        want = model_meta(model)
        if substeps is not None:
            want["substeps"] = int(substeps)
        if statics is not None:
            for key in ("rho", "clip_bound"):
                vals = getattr(statics, key)
                if vals.numel() and bool((vals == vals.reshape(-1)[0]).all()):
                    want[key] = float(vals.reshape(-1)[0])
        for key, val in want.items():
            if key not in self.meta:
                continue
            have = self.meta[key]
            if isinstance(val, (list, tuple)):
                same = len(have) == len(val) and all(abs(float(a) - float(b)) <= 1e-6 * max(1.0, abs(float(b))) for a, b in zip(have, val))
            elif isinstance(val, float):
                same = abs(float(have) - val) <= 1e-6 * max(abs(val), 1e-30)
            else:
                same = have == val
            if not same:
                raise TrajectoryError(f"trajectory meta '{key}' = {have!r} disagrees with the simulator's {val!r}")

    # -- files
    def save(self, path) -> None:
        def cpu(t, dtype=torch.float32):
            return None if t is None else t.detach().to("cpu", dtype).contiguous()
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        torch.save(dict(x=cpu(self.x), v=cpu(self.v), C=cpu(self.C), F=cpu(self.F),
                        mask=None if self.mask is None else (self.mask.detach().cpu() != 0).to(torch.uint8), meta=dict(self.meta)), path)

    @classmethod
    def load(cls, path, device=None) -> 'Trajectory':
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or "x" not in d:
            raise TrajectoryError(f"{path} is not a trajectory file (a dict with 'x')")
        t = cls(d["x"], d.get("v"), d.get("C"), d.get("F"), d.get("mask"), d.get("meta"))       # (validates the shapes)
        return t if device is None else t.to(device)

    @classmethod
    def from_state_folder(cls, folder, meta: Optional[dict] = None) -> 'Trajectory':
        """The NNN.ply clouds that `render -sp` / `inference -sp` write, in frame order, as a position-only trajectory; the first
        cloud is frame 0."""
        from . import io as nio
        files = _state_files(folder)
        clouds = [nio.load_particles_ply(p) for p in files]
        for p, c in zip(files, clouds):
            if c.shape != clouds[0].shape:
                raise TrajectoryError(f"{p.name} has {c.shape[0]} particles, {files[0].name} has {clouds[0].shape[0]}")
        return cls(torch.from_numpy(np.stack(clouds)).float(), meta=meta)


def _state_files(folder):
    files = sorted((p for p in Path(folder).glob("*.ply") if p.stem.isdigit()), key=lambda p: int(p.stem))
    if not files:
        raise TrajectoryError(f"no NNN.ply particle clouds in {folder}")
    return files


class _CloudFrames(object):
    """what `traj.x[f]` is for a CloudTrajectory: f = 0 the initial positions, f >= 1 the observed cloud of frame f"""

    def __init__(self, x0, clouds) -> None:
        self.x0, self.clouds = x0, clouds

    def __len__(self) -> int:
        return len(self.clouds) + 1

    def __getitem__(self, f: int) -> Tensor:
        f = int(f)
        if not 0 <= f <= len(self.clouds):
            raise IndexError(f"frame {f} outside 0..{len(self.clouds)}")
        return self.x0 if f == 0 else self.clouds[f - 1]


class CloudTrajectory(object):
    """Observations that are NOT in the simulator's particle numbering: one unordered cloud per frame, of any size.

        x0 (N, 3)                  the simulated particles' initial positions        required
        v0 (N, 3), C0, F0 (N,3,3)  the rest of the initial state                     optional (zeros / zeros / identity)
        clouds                     T tensors (M_f, 3), M_f >= 1: the cloud of frame f = 1..T
        mask (N)                   rows of x the loss keeps (a surface scan)         optional
        meta                       as Trajectory

    It offers what pretrain.epoch_loss and pretrain_constitutive touch of a Trajectory; only the Chamfer loss can train on it
    (`loss: chamfer`), and there is nothing to teacher-force with.  On disk: one torch.save dict with the keys x0, clouds, ..."""

    can_teacher_force = False
    v = None

    def __init__(self, x0: Tensor, clouds, v0: Optional[Tensor] = None, C0: Optional[Tensor] = None, F0: Optional[Tensor] = None,
                 mask: Optional[Tensor] = None, meta: Optional[dict] = None) -> None:
        self.x0, self.v0, self.C0, self.F0, self.mask = x0, v0, C0, F0, mask
        self.clouds = list(clouds) if isinstance(clouds, (list, tuple)) else clouds
        self.meta = {k: _plain(val) for k, val in dict(meta or {}).items()}
        self.validate()

    @property
    def num_frames(self) -> int:
        return len(self.clouds)

    @property
    def num_particles(self) -> int:
        return int(self.x0.shape[0])

    @property
    def x(self) -> _CloudFrames:
        return _CloudFrames(self.x0, self.clouds)

    def validate(self) -> None:
        x0 = self.x0
        if not isinstance(x0, Tensor) or x0.dim() != 2 or x0.shape[1] != 3 or x0.shape[0] < 1:
            raise TrajectoryError(f"x0 must be (N, 3) with N >= 1, got {tuple(getattr(x0, 'shape', ()))}")
        n = int(x0.shape[0])
        for name, want in (("v0", (n, 3)), ("C0", (n, 3, 3)), ("F0", (n, 3, 3)), ("mask", (n,))):
            t = getattr(self, name)
            if t is not None and tuple(t.shape) != want:
                raise TrajectoryError(f"{name} has shape {tuple(t.shape)}, but x0 {tuple(x0.shape)} asks for {want}")
        if not isinstance(self.clouds, list) or not self.clouds:
            raise TrajectoryError("clouds must be a non-empty list of (M, 3) tensors, one per frame")
        for f, c in enumerate(self.clouds, start=1):
            if not isinstance(c, Tensor) or c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1:
                raise TrajectoryError(f"the cloud of frame {f} must be (M, 3) with M >= 1, got {tuple(getattr(c, 'shape', ()))}")

    def to(self, device) -> 'CloudTrajectory':
        mv = lambda t: None if t is None else t.to(device)      # noqa: E731
        return CloudTrajectory(mv(self.x0), [c.to(device) for c in self.clouds], mv(self.v0), mv(self.C0), mv(self.F0), mv(self.mask),
                               self.meta)

    def frame(self, f: int):
        """(x, v, C, F) of frame f, None for what is not known: the initial state at f = 0, the cloud alone afterwards"""
        return (self.x0, self.v0, self.C0, self.F0) if int(f) == 0 else (self.x[f], None, None, None)

    def forcing_state(self, f: int):
        raise TrajectoryError("teacher forcing needs the full state of every frame in the simulator's particle numbering; "
                              "point-cloud observations have none (teacher_steps must be 0)")

    check_against = Trajectory.check_against

    def save(self, path) -> None:
        def cpu(t):
            return None if t is None else t.detach().to("cpu", torch.float32).contiguous()
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        torch.save(dict(x0=cpu(self.x0), clouds=[cpu(c) for c in self.clouds], v0=cpu(self.v0), C0=cpu(self.C0), F0=cpu(self.F0),
                        mask=None if self.mask is None else (self.mask.detach().cpu() != 0).to(torch.uint8), meta=dict(self.meta)), path)

    @classmethod
    def load(cls, path, device=None) -> 'CloudTrajectory':
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or "x0" not in d or "clouds" not in d:
            raise TrajectoryError(f"{path} is not a point-cloud observation file (a dict with 'x0' and 'clouds')")
        t = cls(d["x0"], d["clouds"], d.get("v0"), d.get("C0"), d.get("F0"), d.get("mask"), d.get("meta"))
        return t if device is None else t.to(device)

    @classmethod
    def from_state_folder(cls, folder, x0: Tensor, v0: Optional[Tensor] = None, C0: Optional[Tensor] = None,
                          F0: Optional[Tensor] = None, mask: Optional[Tensor] = None, meta: Optional[dict] = None) -> 'CloudTrajectory':
        """NNN.ply is the observation of frame NNN, of any size; frames 1..T must all be there.  A 000.ply is allowed and not
        used (the simulation starts from x0)."""
        from . import io as nio
        files = {int(p.stem): p for p in _state_files(folder)}
        files.pop(0, None)
        if not files:
            raise TrajectoryError(f"{folder} holds no observation after frame 0")
        last = max(files)
        missing = [f for f in range(1, last + 1) if f not in files]
        if missing:
            raise TrajectoryError(f"{folder} has no cloud for frame {missing[0]} (frames 1..{last} are needed)")
        clouds = [torch.from_numpy(np.asarray(nio.load_particles_ply(files[f]), dtype=np.float32)) for f in range(1, last + 1)]
        return cls(x0, clouds, v0, C0, F0, mask, meta)


def load_observations(path, x0: Optional[Tensor] = None, **start):
    """A Trajectory or a CloudTrajectory, by what `path` is: a file with 'x' / with 'x0' and 'clouds', or a folder of NNN.ply
    clouds.  The folder becomes a CloudTrajectory when x0 (and optionally v0, C0, F0, mask, meta) is given, else a Trajectory
    (which needs equal sizes)."""
    path = Path(path)
    if path.is_dir():
        if x0 is not None:
            return CloudTrajectory.from_state_folder(path, x0, **start)
        return Trajectory.from_state_folder(path, meta=start.get("meta"))
    d = torch.load(path, map_location="cpu")
    clouds = isinstance(d, dict) and "x0" in d and "clouds" in d
    del d
    return CloudTrajectory.load(path) if clouds else Trajectory.load(path)     # (each load states what its file must hold)
