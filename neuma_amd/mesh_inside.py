"""Particles inside a triangle mesh on the GPU: the ray-parity inside test of extras/mesh_sampling.py (`points_in_mesh`,
`sample_mesh_points`) as one HIP entry point, `nm_points_in_mesh` (csrc/nm_mesh.hip), with the same result bit for bit.
The candidate points and the ray offset come from the extras module's own helpers (`mesh_candidate_points`,
`ray_offset_points`), so both paths test identical fp64 inputs; the extras functions stay the CPU oracle.

prepare.prepare_simulation_data (particle_data.mesh_path) and regist.regist_particles sample through `sample_mesh_points`
here when their device is a GPU.  Inputs and results are numpy arrays; a call uploads the mesh and the points, runs the
kernels on the device's current stream and reads the mask back (one host synchronisation)."""
import numpy as np
import torch

from . import _lib as L
from .extras import mesh_sampling as cpu

_MAX_TRIS = 1 << 27


def _check_mesh(points, verts, tris):
    """(points (n, 3) fp64, verts (v, 3) fp64, tris (m, 3) int32) or ValueError: bad shapes, non-integer or out-of-range
    vertex indices, sizes beyond the C ABI's."""
    p = np.asarray(points, dtype=np.float64)
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tris)
    if t.size == 0:
        t = t.reshape(0, 3)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be (n, 3), got {p.shape}")
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts must be (v, 3), got {v.shape}")
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"tris must be (m, 3), got {t.shape}")
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"tris must hold integer vertex indices, got {t.dtype}")
    if len(p) > np.iinfo(np.int32).max or len(v) > np.iinfo(np.int32).max or len(t) > _MAX_TRIS:
        raise ValueError(f"too large for nm_points_in_mesh: {len(p)} points, {len(v)} vertices, {len(t)} triangles")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= len(v)):
        raise ValueError(f"vertex index out of range [0, {len(v)}): min {int(t.min())}, max {int(t.max())}")
    return p, v, t.astype(np.int32)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.NeumaHipError("mesh_inside runs on the GPU (extras.mesh_sampling is the CPU path)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def inside_native(points: torch.Tensor, verts: torch.Tensor, tris: torch.Tensor) -> torch.Tensor:
    """One nm_points_in_mesh call on device tensors: points (n, 3) fp64 that already carry the ray offset, verts (v, 3) fp64,
    tris (m, 3) int32 with indices in [0, v).  Returns (n,) uint8 on the device (1 = inside); no host synchronisation."""
    for name, t, dt in (("points", points, torch.float64), ("verts", verts, torch.float64), ("tris", tris, torch.int32)):
        if not (t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous (n, 3) {dt} GPU tensor, got {tuple(t.shape)} {t.dtype} on {t.device}")
    dev = L.same_device(points, verts, tris)
    lib = L.lib()
    n, nv, nt = int(points.shape[0]), int(verts.shape[0]), int(tris.shape[0])
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(int(lib.nm_mesh_inside_workspace(nt, n)), 1), dtype=torch.uint8, device=dev)
    L.check(lib.nm_points_in_mesh(nv, nt, n, verts.data_ptr(), tris.data_ptr(), points.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), L.stream_ptr(dev)), "nm_points_in_mesh")
    return out


def points_in_mesh(points, verts, tris, device="cuda") -> np.ndarray:
    """extras.mesh_sampling.points_in_mesh on the GPU: bool (n,), True where the +z ray from the (offset) point crosses the
    mesh an odd number of times.  Same result bit for bit; an out-of-range vertex index raises ValueError here (numpy would
    wrap a negative one)."""
    p, v, t = _check_mesh(points, verts, tris)
    if len(p) == 0 or len(t) == 0:
        return np.zeros(len(p), dtype=bool)
    dev = _device(device)
    q = cpu.ray_offset_points(p, v)
    out = inside_native(torch.from_numpy(np.ascontiguousarray(q)).to(dev), torch.from_numpy(np.ascontiguousarray(v)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(t)).to(dev))
    return out.cpu().numpy().astype(bool)


def sample_mesh_points(verts, tris, mode: str = "volumetric", resolution: int = 30, seed: int = 0, device="cuda") -> np.ndarray:
    """extras.mesh_sampling.sample_mesh_points on the GPU: the same candidates ('volumetric' lattice or seeded 'uniform'
    points), the inside ones kept in the same order."""
    pts = cpu.mesh_candidate_points(verts, mode, resolution, seed)
    return pts[points_in_mesh(pts, verts, tris, device)]
