"""Signed distance fields of closed triangle meshes on the GPU (no reference counterpart): the unsigned distance of every
lattice node by `nm_mesh_distance` (csrc/nm_sdf.hip), the sign by the existing point-in-mesh kernel (neuma_amd/mesh_inside.py).
The definition - lattice, per-triangle formula, dropped and degenerate triangles, closedness - is neuma_amd/extras/mesh_sdf.py,
which is also the CPU path (`device="cpu"`) and supplies the lattice and the mesh checks to both.

    field = build_mesh_field(verts, tris, resolution=64)          # MeshField(phi (nx, ny, nz) fp32 on the device, origin, spacing, dims)

The triangles are uploaded in a fixed pseudo-random order (extras.mesh_sdf.cull_order): the field does not depend on the order,
the kernel's bounding-sphere cull does.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import mesh_inside
from .extras import mesh_sdf as cpu
from .extras.mesh_sdf import MeshField      # noqa: F401  (re-exported)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.NeumaHipError("mesh_sdf.mesh_distance runs on the GPU (extras.mesh_sdf is the CPU path)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def distance_native(verts: torch.Tensor, tris: torch.Tensor, origin, spacing: float, dims, out: torch.Tensor = None) -> torch.Tensor:
    """One nm_mesh_distance call on device tensors: verts (v, 3) fp32, tris (m, 3) int32 (any indices: out-of-range ones drop
    their triangle).  Returns (nx, ny, nz) fp32 on the device; no host synchronisation."""
    for name, t, dt in (("verts", verts, torch.float32), ("tris", tris, torch.int32)):
        if not (t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous (n, 3) {dt} GPU tensor, got {tuple(t.shape)} {t.dtype} on {t.device}")
    dev = L.same_device(verts, tris, out)
    lib = L.lib()
    d = tuple(int(x) for x in dims)
    if len(d) != 3:
        raise ValueError(f"dims: three lattice sizes expected, got {dims!r}")
    nodes = d[0] * d[1] * d[2]
    if out is None:
        out = torch.empty(tuple(max(x, 0) for x in d), dtype=torch.float32, device=dev)
    elif not (out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= max(nodes, 0)):
        raise ValueError("out: a contiguous fp32 tensor of prod(dims) elements expected")
    nv, nt = int(verts.shape[0]), int(tris.shape[0])
    ws = torch.empty(max(int(lib.nm_mesh_distance_workspace(nt, max(nodes, 0))), 1), dtype=torch.uint8, device=dev)
    o = (C.c_float * 3)(*(float(x) for x in origin))
    dd = (C.c_int32 * 3)(*d)
    L.check(lib.nm_mesh_distance(nv, nt, verts.data_ptr(), tris.data_ptr(), o, float(spacing), dd, out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), L.stream_ptr(dev)), "nm_mesh_distance")
    return out


def mesh_distance(verts, tris, origin, spacing, dims, device="cuda") -> torch.Tensor:
    """extras.mesh_sdf.mesh_distance on the GPU, in fp32: (nx, ny, nz) on the device.  numpy inputs; the triangles are uploaded
    in cull_order."""
    dev = _device(device)
    d = cpu.check_lattice(spacing, dims)
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
    t = np.asarray(tris)
    t = t.reshape(-1, 3) if t.size else np.zeros((0, 3), dtype=np.int64)
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"tris must hold integer vertex indices, got {t.dtype}")
    if len(t) > cpu.MAX_TRIS:
        raise ValueError(f"too many triangles for nm_mesh_distance: {len(t)} > 2^24")
    t = np.clip(t, -1, np.iinfo(np.int32).max)[cpu.cull_order(len(t))].astype(np.int32)
    return distance_native(torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(t).reshape(-1, 3)).to(dev),
                           np.asarray(origin, dtype=np.float32), float(np.float32(spacing)), d)


def build_mesh_field(verts, tris, spacing=None, resolution: int = 64, margin_cells: int = 2, device="cuda") -> MeshField:
    """The signed distance field of a closed triangle mesh: the lattice is the mesh's bounding box grown by `margin_cells` cells
    on every side (`resolution` cells along the longest axis when `spacing` is None); phi = -dist where
    mesh_inside.points_in_mesh calls the node inside, +dist elsewhere.  ValueError for a mesh that is not closed (the count of
    offending edges) or inverted (mesh_volume not positive).  device: a GPU -> phi is an fp32 tensor there; "cpu" -> the numpy
    fp64 path of extras.mesh_sdf."""
    if torch.device(device).type != "cuda":
        return cpu.build_mesh_field(verts, tris, spacing, resolution, margin_cells)
    dev = _device(device)
    t = cpu.check_closed_mesh(verts, tris)
    origin, h, dims = cpu.field_lattice(verts, spacing, resolution, margin_cells)
    dist = mesh_distance(verts, t, origin, h, dims, dev)
    v64 = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    inside = mesh_inside.points_in_mesh(cpu.lattice_nodes(origin, h, dims).reshape(-1, 3), v64, t, dev)
    phi = torch.where(torch.from_numpy(inside.reshape(dims)).to(dev), -dist, dist)
    return MeshField(phi, tuple(float(x) for x in origin), float(h), dims)
