"""Recorded particle trajectories: the targets of constitutive pretraining (pretrain.py).

A Trajectory holds T + 1 frames of N particles, frame 0 being the initial state:

    x (T+1, N, 3)            positions                          required
    v (T+1, N, 3)            velocities                         optional (without it the supervision is position-only)
    C, F (T+1, N, 3, 3)      affine momentum, deformation       optional, only together (needed for teacher forcing)
    mask (N)                 rows the loss keeps                optional
    meta                     the simulator the frames came from: MODEL_KEYS (what MPMModelBuilder.parse_cfg consumes) plus
                             substeps per frame, and rho / clip_bound of the particles

On disk it is one torch.save dict of CPU fp32 tensors (mask: uint8) and plain-Python meta.  The reference has no counterpart."""
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
        files = sorted((p for p in Path(folder).glob("*.ply") if p.stem.isdigit()), key=lambda p: int(p.stem))
        if not files:
            raise TrajectoryError(f"no NNN.ply particle clouds in {folder}")
        clouds = [nio.load_particles_ply(p) for p in files]
        for p, c in zip(files, clouds):
            if c.shape != clouds[0].shape:
                raise TrajectoryError(f"{p.name} has {c.shape[0]} particles, {files[0].name} has {clouds[0].shape[0]}")
        return cls(torch.from_numpy(np.stack(clouds)).float(), meta=meta)
