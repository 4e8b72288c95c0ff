"""Contact forces of a roll-out on the per-operator MPM path: how hard the body presses on the box walls and on each collider,
frame by frame.  No reference counterpart.  Definition of a substep's rows: include/neuma_hip.h "Contact report"; fp64
restatement: neuma_amd/extras/contact.py; kernels: csrc/nm_contact.h + k_contact_rows / k_contact_sum (MPMModel.contact()).

    meter = ContactMeter(model)
    for every substep:   sim(statics, state); meter.record(); model.step_colliders()
    for every frame:     meter.frame()
    meter.write_csv(path); print(meter.summary())

record() keeps the substep's rows on the device together with the torque impulse about each obstacle's reference point AS IT IS
THEN - the plane's point, the centre of a sphere or box (a rigid body's: its centre on the device at that substep), the lattice
centre of a field collider, the simulation origin for the walls - which is why it comes before step_colliders().  frame() sums the
substeps since the last frame and divides by the simulated time they cover: F = sum J / T, torque = sum (L - r0 x J) / T, normal =
sum N / T (the mean normal force); mass and nodes are means over the frame's substeps. Nothing is read back to the host before
write_csv() / summary(). Simulation units throughout (the unit cube, rho * vol masses): no conversion to world units.

`--report_contacts` on `python -m neuma_amd.render` / `python -m neuma_amd.inference` (or `sim.report_contacts: true`) runs a
meter with one substep per frame and writes <result dir>/contacts_<video_name>.csv.
"""
import csv
from pathlib import Path
from typing import List, Optional

import torch

from .sim.colliders import Plane
from .sim.mpm import ContactReport

CSV_COLUMNS = ("frame", "time", "row", "name", "Fx", "Fy", "Fz", "Tx", "Ty", "Tz", "normal", "mass", "nodes")


def wanted(cfg, sim_cfg) -> bool:
    """--report_contacts on the command line or `sim.report_contacts: true` in the config"""
    return bool(cfg.get("report_contacts", False) or (sim_cfg is not None and sim_cfg.get("report_contacts", False)))


def reference_points(model) -> List[tuple]:
    """One torque reference per row of model.contact(), where the obstacles are NOW: the origin for the walls, a plane's point, the
    centre of a sphere or box, the centre of a field collider's lattice."""
    pts = [(0.0, 0.0, 0.0)]
    # (with rigid bodies: the list the host holds, without a read-back - a body's entry is where it started, and reference_tensor
    #  puts its centre in.  getattr: the meter also serves stand-ins of a model that have `colliders` and nothing newer)
    for c in (model.prescribed_colliders if getattr(model, "rigid_bodies", None) else model.colliders):
        pts.append(tuple(c.point if isinstance(c, Plane) else c.center))
    for c in model.field_colliders:
        pts.append(tuple(o + 0.5 * (d - 1) * c.spacing for o, d in zip(c.origin, c.dims)))
    return pts


def reference_tensor(model, like: torch.Tensor) -> torch.Tensor:
    """reference_points as an (R, 3) tensor like `like`, the rows of rigid bodies taken from the centres of model.rigid_state() on
    the device: nothing is read back"""
    pts = torch.as_tensor(reference_points(model), dtype=like.dtype, device=like.device)
    bodies = model.rigid_bodies
    if bodies:
        pts[torch.as_tensor([1 + i for i, _ in bodies], device=like.device)] = model.rigid_state()[:, 0:3].to(like.dtype)
    return pts


def shifted(angular: torch.Tensor, impulse: torch.Tensor, about) -> torch.Tensor:
    """L - r0 x J per row: the angular impulse about the points `about` (R, 3) instead of the origin"""
    r0 = torch.as_tensor(about, dtype=angular.dtype, device=angular.device).expand_as(impulse)
    return angular - torch.linalg.cross(r0, impulse)


class ContactMeter(object):
    def __init__(self, model, dt: Optional[float] = None) -> None:
        self.model = model
        self.dt = float(model.constant.dt if dt is None else dt)
        self.names = None
        self.time = 0.0
        self._open = []          # substeps since the last frame: (rows (R, 9), torque impulse about the references (R, 3))
        self.frames = []         # closed frames: (time at their end, elapsed, substeps, rows sum (R, 9), torque impulse sum (R, 3))
        self._host = None        # write_csv / summary: the closed frames on the host, read back once

    def record(self, report: Optional[ContactReport] = None) -> ContactReport:
        """Take the last substep's rows (model.contact(), or the given report).  Before model.step_colliders()."""
        rep = self.model.contact() if report is None else report
        if self.names is None:
            self.names = list(rep.names)
        about = reference_tensor(self.model, rep.rows) if getattr(self.model, "rigid_bodies", None) else reference_points(self.model)
        self._open.append((rep.rows, shifted(rep.angular, rep.impulse, about)))
        return rep

    def frame(self) -> ContactReport:
        """Close a frame over the substeps recorded since the last one; returns their summed rows."""
        if not self._open:
            raise ValueError("contact: frame() without a recorded substep")
        rows = torch.stack([r for r, _ in self._open]).sum(0) if len(self._open) > 1 else self._open[0][0]
        tq = torch.stack([t for _, t in self._open]).sum(0) if len(self._open) > 1 else self._open[0][1]
        elapsed = len(self._open) * self.dt
        self.time += elapsed
        self.frames.append((self.time, elapsed, len(self._open), rows, tq))
        self._open, self._host = [], None
        return ContactReport(rows, self.names)

    def _table(self):
        """per closed frame (time, F (R, 3), T (R, 3), normal (R,), mass (R,), nodes (R,)) on the host: the one read-back"""
        if self._host is None and self.frames:
            rows = torch.stack([f[3] for f in self.frames]).cpu()
            tq = torch.stack([f[4] for f in self.frames]).cpu()
            self._host = []
            for (time, elapsed, subs, _, _), r, t in zip(self.frames, rows, tq):
                self._host.append((time, r[:, 0:3] / elapsed, t / elapsed, r[:, 6] / elapsed, r[:, 7] / subs, r[:, 8] / subs, r[:, 0:3]))
        return self._host or []

    def write_csv(self, path) -> Path:
        """One line per frame and row (CSV_COLUMNS), frames counted from 1."""
        path = Path(path)
        with open(path, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(CSV_COLUMNS)
            for k, (time, F, T, normal, mass, nodes, _) in enumerate(self._table(), start=1):
                for r, name in enumerate(self.names):
                    w.writerow([k, repr(float(time)), r, name] + [repr(float(a)) for a in (*F[r], *T[r], normal[r], mass[r], nodes[r])])
        return path

    def summary(self) -> str:
        """Per row: the peak |F| and its frame, and the total impulse."""
        table = self._table()
        if not table:
            return "contacts: no frame recorded"
        lines = [f"contacts: {len(table)} frames, simulation units"]
        mag = torch.stack([t[1].norm(dim=-1) for t in table])          # (frames, R)
        total = torch.stack([t[6] for t in table]).sum(0)              # (R, 3)
        for r, name in enumerate(self.names):
            k = int(torch.argmax(mag[:, r]))
            J = ", ".join(f"{float(a):.6g}" for a in total[r])
            lines.append(f"  {name}: peak |F| = {float(mag[k, r]):.6g} at frame {k + 1}, total impulse = ({J})")
        return "\n".join(lines)
