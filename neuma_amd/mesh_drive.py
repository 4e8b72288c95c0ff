"""A user's triangle mesh driven by the roll-out (no reference counterpart): the same vertices in the same order, the same faces,
UVs and materials untouched, only the positions move - what a DCC tool imports as a vertex animation, and what `--save_mesh`
(a new surface per frame, no correspondence) cannot give.  extras/mesh_drive.py states the definition (an affine
moving-least-squares fit over each vertex's k nearest rest particles, written as fixed coefficients) and is the CPU path; on the
GPU the search is nm_knn, the fit and the vertex normals are csrc/nm_meshdrive.hip (nm_mesh_bind, nm_mesh_normals), a frame's
positions are one nm_bind_frame launch over the coefficient rows (V0 + C (x - X)) and vertex colours are nm_field_paint over
the weight rows.

    MeshDriver(vertices, triangles, rest_particles, k=16, damping=1e-5, device="cuda")
        .frame(particles, values=None, value_range=None, colormap=None) -> (positions, normals[, rgb])
        .describe()

    python -m neuma_amd.mesh_drive --mesh M.{obj,ply} --rest particles0.ply --states DIR -o OUT [--k K] [--damping E]
        [--format ply|obj] [--device cuda|cpu]

drives M from any folder of same-ordered NNN.ply particle clouds (`render --save_particles`) into OUT/NNN.{ply,obj}; one line per
frame: V, T and the largest edge-length ratio to rest.  `obj` on an .obj input keeps every line of the source file but the `v`
positions, the dropped `vn` lines and the faces' normal indices."""
import argparse
import sys
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from .extras import mesh_drive as cpu

C0 = 0.28209479177387814


def read_mesh(path) -> Tuple[np.ndarray, np.ndarray, Optional[str]]:
    """(vertices (V, 3) fp64, triangles (T, 3) int64, the OBJ text or None) of an .obj or .ply mesh file."""
    path = Path(path)
    if path.suffix.lower() == ".obj":
        text = path.read_bytes().decode("utf-8", "surrogateescape")
        v, t = cpu.read_obj(text)
        return v, t, text
    from .io import read_ply_mesh
    v, t = read_ply_mesh(path)
    return v, t, None


def _rows(rowptr, col, val, K, N):
    """the constant-k CSR as the tune.Bindings field_paint reads (forward rows only)"""
    from .tune import Bindings
    b = Bindings.__new__(Bindings)
    b.K, b.N, b.nnz, b.rowptr, b.col, b.val = K, N, int(val.numel()), rowptr, col, val
    return b


class MeshDriver(object):
    """Binds a mesh (vertices (V, 3), triangles (T, 3), in the frame of `rest_particles` (N, 3)) once: the neighbour search, the
    coefficients and the corner adjacency.  `frame` then gives the mesh for any state of the same particles.  device "cpu" runs
    the fp64 definition (extras/mesh_drive.py) and returns CPU tensors.  ValueError: non-finite vertices or particles, a triangle
    index outside [0, V), k outside 1..16 or above N, damping <= 0, V k >= 2^31, and in `frame` a changed particle count or
    non-finite particles."""

    def __init__(self, vertices, triangles, rest_particles, k: int = cpu.DEFAULT_K, damping: float = cpu.DEFAULT_DAMPING, device="cuda"):
        as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        V0 = cpu._f32_as_f64(as_np(vertices), "vertices").astype(np.float32)
        X = cpu._f32_as_f64(as_np(rest_particles), "rest particles").astype(np.float32)
        self.k, self.damping = cpu.check_k(k, len(X), damping)
        self.V, self.N = len(V0), len(X)
        if self.V * self.k >= 2 ** 31:
            raise ValueError(f"{self.V} vertices x k = {self.k} does not fit an int32")
        tri = cpu.check_triangles(as_np(triangles), self.V)
        self.T = len(tri)
        vptr, vcorner = cpu.corner_adjacency(tri, self.V)
        self.device = torch.device(device)
        self.triangles_np, self.vertices_np = tri, V0
        if self.device.type != "cuda":
            idx, d2 = cpu.knn_brute(V0, X, self.k)
            self._col, self._c, self._w, _ = cpu.bind(V0, X, idx, d2, self.damping)
            self._X, self._vptr, self._vcorner = X, vptr, vcorner
            self._info = cpu.describe(self.V, self.T, self.k, self._c, d2)
            return
        from . import _lib as L
        from .particle_metrics import k_nearest_neighbors
        dev = self.device
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.vertices, self.rest, self.triangles = put(V0), put(X), put(tri)
        self.vptr, self.vcorner = put(vptr), put(vcorner)
        self.col = torch.empty(self.V, self.k, dtype=torch.int32, device=dev)
        self.coeff = torch.empty(self.V, self.k, dtype=torch.float32, device=dev)
        self.weight = torch.empty(self.V, self.k, dtype=torch.float32, device=dev)
        self.rowptr = (torch.arange(self.V + 1, dtype=torch.int64, device=dev) * self.k).to(torch.int32)
        d2 = torch.empty(0, self.k, dtype=torch.float64, device=dev)
        if self.V:
            idx, d2 = k_nearest_neighbors(self.vertices[None], self.rest[None], self.k)
            self.idx, self.d2 = idx[0], d2[0]
            L.check(L.lib().nm_mesh_bind(self.V, self.N, self.k, self.damping, L.ptr(self.vertices), L.ptr(self.rest), self.idx.data_ptr(),
                                         self.d2.data_ptr(), L.ptr(self.col), L.ptr(self.coeff), L.ptr(self.weight), L.stream_ptr(dev)),
                    "nm_mesh_bind")
            d2 = self.d2
        self._paint_rows = _rows(self.rowptr, self.col.reshape(-1), self.weight.reshape(-1), self.V, self.N)
        self._info = cpu.describe(self.V, self.T, self.k, self.coeff.cpu().numpy(), d2.cpu().numpy())       # the one read-back, at bind

    def describe(self) -> str:
        i = self._info
        return (f"mesh drive: V = {i['V']}, T = {i['T']}, k = {i['k']}, max sum|c| = {i['max_abs_c']:.3g}, "
                f"farthest nearest particle / median = {i['far']:.3g}")

    def normals(self, positions: torch.Tensor) -> torch.Tensor:
        """nm_mesh_normals of `positions` (V, 3) on the driver's triangles."""
        if self.device.type != "cuda":
            return torch.from_numpy(cpu.normals(positions.numpy(), self.triangles_np, self._vptr, self._vcorner).astype(np.float32))
        from . import _lib as L
        out = torch.empty(self.V, 3, dtype=torch.float32, device=self.device)
        L.check(L.lib().nm_mesh_normals(self.V, self.T, L.ptr(positions, torch.float32), L.ptr(self.triangles) if self.T else None,
                                        L.ptr(self.vptr), L.ptr(self.vcorner) if self.T else None, L.ptr(out), L.stream_ptr(self.device)),
                "nm_mesh_normals")
        return out

    def _particles(self, particles) -> torch.Tensor:
        x = particles if torch.is_tensor(particles) else torch.as_tensor(np.asarray(particles))
        if x.dim() != 2 or tuple(x.shape) != (self.N, 3):
            raise ValueError(f"particles: shape ({self.N}, 3) expected (the mesh is bound to {self.N} particles), got {tuple(x.shape)}")
        x = x.detach().to(self.device, torch.float32).contiguous()
        if not bool(torch.isfinite(x).all()):
            raise ValueError("particles: non-finite values")
        return x

    def frame(self, particles, values=None, value_range=None, colormap=None):
        """(positions (V, 3), normals (V, 3)) fp32 on the driver's device for the particle state `particles` (N, 3), and with
        `values` (N,) also rgb (V, 3) in [0, 1]: the w^-weighted mean of the neighbours' values through `colormap` (default
        "heat") over `value_range` ((lo, hi) numbers, 2 device floats as field_paint keeps them, or None: the range of the
        vertex values)."""
        x = self._particles(particles)
        if self.device.type != "cuda":
            pos = torch.from_numpy(cpu.drive(self.vertices_np, self._col, self._c, self._X, x.numpy()).astype(np.float32))
            out = (pos, self.normals(pos))
            if values is None:
                return out
            from .extras import field_paint as fp
            q = values.detach().cpu().double().reshape(-1).numpy() if torch.is_tensor(values) else np.asarray(values, dtype=np.float64).reshape(-1)
            if len(q) != self.N:
                raise ValueError(f"values: {self.N} expected, got {len(q)}")
            g = torch.from_numpy(cpu.vertex_values(self._w, self._col, q))
            rng = tuple(float(a) for a in value_range) if value_range is not None else fp.data_range(g)
            return out + (fp.colors(g, rng, colormap or "heat").float(),)
        from . import _lib as L
        pos = torch.empty(self.V, 3, dtype=torch.float32, device=self.device)
        L.check(L.lib().nm_bind_frame(self.V, L.ptr(self.rowptr), L.ptr(self.col), L.ptr(self.coeff), L.ptr(x), L.ptr(self.rest),
                                      L.ptr(self.vertices), None, None, L.ptr(pos), None, None, L.stream_ptr(self.device)), "nm_bind_frame")
        out = (pos, self.normals(pos))
        if values is None:
            return out
        from . import field_paint
        q = values.detach().to(self.device, torch.float32).reshape(-1)
        if q.numel() != self.N:
            raise ValueError(f"values: {self.N} expected, got {q.numel()}")
        cmap = colormap or "heat"
        if torch.is_tensor(value_range):
            dc, _ = field_paint.paint_raw(q, self._paint_rows, cmap, value_range, want_g=False)
        elif value_range is not None:
            r = torch.tensor(field_paint.check_range(value_range), dtype=torch.float32, device=self.device)
            dc, _ = field_paint.paint_raw(q, self._paint_rows, cmap, r, want_g=False)
        else:
            _, g = field_paint.paint_raw(q, self._paint_rows, want_dc=False)
            dc, _ = field_paint.paint_raw(g, None, cmap, field_paint.field_range(g), want_g=False)
        return out + ((0.5 + C0 * dc).clamp(0.0, 1.0),)

    def rest_frame(self):
        """(positions, normals) of the bound mesh itself: what an object that has not joined the roll-out yet is written as"""
        pos = self.vertices if self.device.type == "cuda" else torch.from_numpy(self.vertices_np)
        return pos, self.normals(pos)


def save_frame(path, positions, normals, colors, triangles, fmt: str = "ply", obj_text: Optional[str] = None) -> None:
    """One driven frame: binary PLY (io.save_mesh_ply), or OBJ - the source text rewritten (extras.rewrite_obj) when the mesh came
    from an .obj, io.save_mesh_obj otherwise."""
    from . import io as nio
    to_np = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
    p, n, c, t = to_np(positions), to_np(normals), to_np(colors), to_np(triangles)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    if fmt == "obj" and obj_text is not None:
        Path(path).write_bytes(cpu.rewrite_obj(obj_text, p).encode("utf-8", "surrogateescape"))
    elif fmt == "obj":
        nio.save_mesh_obj(path, p, n, c, t)
    else:
        nio.save_mesh_ply(path, p, n, c, t)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drive a triangle mesh with a folder of same-ordered particle clouds.")
    p.add_argument("--mesh", type=str, required=True, help="the mesh (.obj or .ply), in the frame of the rest particles")
    p.add_argument("--rest", type=str, required=True, help="the rest particle cloud (.ply) the mesh is bound to")
    p.add_argument("--states", type=str, required=True, help="folder of NNN.ply particle clouds in the order of --rest")
    p.add_argument("--output", "-o", type=str, required=True, help="folder of NNN.{ply,obj} driven meshes")
    p.add_argument("--k", type=int, default=cpu.DEFAULT_K, help="neighbours per vertex, 1..16")
    p.add_argument("--damping", type=float, default=cpu.DEFAULT_DAMPING)
    p.add_argument("--format", type=str, default="ply", choices=("ply", "obj"))
    p.add_argument("--device", type=str, default="cuda", choices=("cuda", "cpu"))
    return p.parse_args(argv)


@torch.no_grad()
def main(argv=None):
    from . import io as nio
    args = parse_args(argv)
    verts, tris, text = read_mesh(args.mesh)
    rest = nio.load_particles_ply(args.rest)
    driver = MeshDriver(verts, tris, rest, args.k, args.damping, args.device)
    print(driver.describe())
    frames = sorted((p for p in Path(args.states).glob("*.ply") if p.stem.isdigit()), key=lambda p: int(p.stem))
    if not frames:
        raise FileNotFoundError(f"no NNN.ply frames in {args.states}")
    out = Path(args.output)
    out.mkdir(parents=True, exist_ok=True)
    for src in frames:
        pos, nrm = driver.frame(nio.load_particles_ply(src))
        dst = out / f"{src.stem}.{args.format}"
        save_frame(dst, pos, nrm, None, driver.triangles_np, args.format, text)
        ratio = cpu.edge_ratio(pos.cpu().numpy(), driver.vertices_np, driver.triangles_np)
        print(f"{src.name}: V = {driver.V}, T = {driver.T}, largest edge / rest = {ratio:.6g} -> [{dst}]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
