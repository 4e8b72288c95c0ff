"""Rigid bodies of a roll-out on the per-operator MPM path: where every body is, frame by frame, and whether the explicit coupling
was asked for more than it can give.  No reference counterpart.  Definition: include/neuma_hip.h "Rigid bodies"; fp64 restatement:
neuma_amd/extras/rigid.py; kernels: csrc/nm_rigid.h (MPMModel.step_colliders() -> nm_mpm_rigid_step).

    log = RigidLog(model)
    for every substep:   sim(statics, state); model.step_colliders(); log.after_step()
    log.write_csv(path); for line in log.mass_ratio_notes(): print(line)

after_step keeps the bodies' states (MPMModel.rigid_state()) and the `mass` column of the contact rows the step consumed
(MPMModel.rigid_rows(): a copy, no second reduction), both on the device: nothing is read back before write_csv() /
mass_ratio_notes().  One frame per recorded substep, as the drivers run one substep per frame.

A sticky body changes its velocity by (sum m_i / M)(u_mean - v) per substep, sum m_i that mass column: beyond a ratio of 1 the step
overshoots, beyond 2 it diverges.  Nothing enforces the limit; mass_ratio_notes() says which body exceeded 1, and when.

`python -m neuma_amd.render` / `python -m neuma_amd.inference` write <result dir>/rigid_<video_name>.csv whenever `sim.colliders`
holds a body.  Simulation units throughout (the unit cube, rho * vol masses)."""
import csv
from pathlib import Path
from typing import List

import torch

CSV_COLUMNS = ("frame", "time", "body", "cx", "cy", "cz", "qw", "qx", "qy", "qz", "vx", "vy", "vz", "wx", "wy", "wz")


class RigidLog(object):
    def __init__(self, model) -> None:
        self.model = model
        self.dt = float(model.constant.dt)
        self.bodies = model.rigid_bodies                # [(collider index, RigidBody)]
        self.names = [f"{i}:{type(model.prescribed_colliders[i]).__name__.lower()}" for i, _ in self.bodies]
        self._rows = torch.as_tensor([1 + i for i, _ in self.bodies], dtype=torch.int64)
        self._mass = []      # per substep: (bodies,) contact mass, on the device
        self._state = []     # per substep: (bodies, 19), on the device

    def after_step(self) -> None:
        """The bodies' states and the contact mass each was just moved by.  After model.step_colliders()."""
        rows = self.model.rigid_rows()
        self._mass.append(rows[self._rows.to(rows.device), 7])
        self._state.append(self.model.rigid_state())

    def write_csv(self, path) -> Path:
        """One line per frame and body (CSV_COLUMNS), frames counted from 1, the state at the end of the frame."""
        path = Path(path)
        states = torch.stack(self._state).cpu() if self._state else torch.zeros(0, len(self.bodies), 19, dtype=torch.float64)
        with open(path, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(CSV_COLUMNS)
            for k, frame in enumerate(states, start=1):
                for name, row in zip(self.names, frame):
                    w.writerow([k, repr(k * self.dt), name] + [repr(float(a)) for a in (*row[0:7], *row[13:19])])
        return path

    def mass_ratio_notes(self) -> List[str]:
        """One line per body whose peak contact mass / M exceeded 1, naming the frame."""
        if not self._mass:
            return []
        ratio = torch.stack(self._mass).cpu() / torch.as_tensor([b.mass for _, b in self.bodies], dtype=torch.float64)
        lines = []
        for j, name in enumerate(self.names):
            k = int(torch.argmax(ratio[:, j]))
            peak = float(ratio[k, j])
            if peak > 1.0 and not self.bodies[j][1].kinematic:
                what = "diverges beyond 2" if peak > 2.0 else "overshoots"
                lines.append(f"rigid body {name}: peak contact mass / M = {peak:.4g} at frame {k + 1} (> 1: the explicit coupling "
                             f"{what}; use a heavier body or a smaller dt)")
        return lines
