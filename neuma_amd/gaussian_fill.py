"""Particles out of the Gaussians' own density field: what `prepare` needs between `reconstruct` (kernels.ply) and
`finetune` when there is neither a particle cloud nor a watertight mesh.  The opacity density of the fitted Gaussians is
evaluated on a lattice, thresholded into a surface shell, the cells the shell encloses are marked (six-ray test), and
particles are emitted in both.  extras/gaussian_fill.py states the algorithm, computes the lattice for both paths and is
the CPU path; here it runs as HIP kernels (csrc/nm_fill.hip): the density as a gather by 4^3 block over sorted
(block, Gaussian) pairs - no float atomics, so two runs give identical bytes - and the classification and emission as
integer passes that equal the numpy ones bit for bit on any field.

    python -m neuma_amd.gaussian_fill -k kernels.ply -o particles.ply [--sh_degree D] [--resolution R]
        [--density_thres T] [--cutoff C] [--per_cell N] [--no_shell] [--opacity_thres 0.02] [--device cuda]

`density_thres` = 0.5 is a default nobody has tuned on a real capture yet."""
import argparse
import ctypes as C
import sys
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib as L
from .extras import gaussian_fill as cpu


def _lattice_args(origin, h, dims):
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    d = [int(x) for x in np.asarray(dims).reshape(3)]
    if min(d) < 1 or d[0] * d[1] * d[2] > cpu.MAX_CELLS:
        raise ValueError(f"lattice dims {d} must be >= 1 and hold at most 2^27 cells")
    if not (np.isfinite(o).all() and np.isfinite(h) and h > 0):
        raise ValueError("lattice origin / cell edge must be finite, the edge positive")
    return (C.c_double * 3)(*o), float(h), (C.c_int32 * 3)(*d), d


def _gpu(name, t, dtype, shape_tail):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape[1:]) == shape_tail):
        raise ValueError(f"{name}: expected a contiguous (n{''.join(', %d' % s for s in shape_tail)}) {dtype} GPU tensor, got "
                         f"{tuple(t.shape)} {t.dtype} on {t.device}")


def density_field(means: torch.Tensor, cov6: torch.Tensor, opacity: torch.Tensor, origin, h, dims, cutoff: float = 9.0
                  ) -> Tuple[torch.Tensor, int]:
    """(field (ncells,) fp32 on the device, number of degenerate Gaussians skipped) for device tensors means (K, 3), cov6
    (K, 6), opacity (K,), all finite fp32, on the lattice of extras.gaussian_fill.fill_lattice.  One host read-back (the
    pair count sizes the workspace).  Two calls on the same input give identical bytes."""
    _gpu("means", means, torch.float32, (3,))
    _gpu("cov6", cov6, torch.float32, (6,))
    opacity = opacity.reshape(-1)
    _gpu("opacity", opacity, torch.float32, ())
    K = int(means.shape[0])
    if K == 0 or cov6.shape[0] != K or opacity.shape[0] != K:
        raise ValueError(f"means, cov6 and opacity must hold the same K >= 1 Gaussians, got {K}, {cov6.shape[0]}, {opacity.shape[0]}")
    dev = L.same_device(means, cov6, opacity)
    o, h, d, dl = _lattice_args(origin, h, dims)
    cutoff = cpu._cutoff(cutoff)
    lib, stream = L.lib(), L.stream_ptr(dev)
    g10 = torch.empty((K, 10), dtype=torch.float32, device=dev)
    boxes = torch.empty((K, 6), dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(lib.nm_fill_gaussians(K, means.data_ptr(), cov6.data_ptr(), opacity.data_ptr(), o, h, d, cutoff, g10.data_ptr(),
                                  boxes.data_ptr(), counts.data_ptr(), totals.data_ptr(), stream), "nm_fill_gaussians")
    n_pairs, n_skipped = (int(v) for v in totals.cpu())
    if n_pairs > np.iinfo(np.int32).max:
        raise ValueError(f"{n_pairs} (Gaussian, block) pairs do not fit an int32: lower `resolution` or prune large Gaussians")
    n_blocks = int(np.prod([(x + cpu.BLOCK - 1) // cpu.BLOCK for x in dl]))
    ws_bytes = int(lib.nm_fill_density_workspace(K, n_pairs, n_blocks))
    if ws_bytes == 0:
        raise L.NeumaHipError(f"nm_fill_density_workspace rejects K={K}, pairs={n_pairs}, blocks={n_blocks}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    field = torch.empty(dl[0] * dl[1] * dl[2], dtype=torch.float32, device=dev)
    L.check(lib.nm_fill_density(K, n_pairs, g10.data_ptr(), boxes.data_ptr(), counts.data_ptr(), o, h, d, cutoff, field.data_ptr(),
                                ws.data_ptr(), ws.numel(), stream), "nm_fill_density")
    return field, n_skipped


def classify_emit(field: torch.Tensor, origin, h, dims, density_thres: float = 0.5, per_cell: int = 1, include_shell: bool = True
                  ) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """(points (M, 3) fp32, kind (M,) uint8, counts) on the device from ANY fp32 field (ncells,) on the device: the integer
    stage, equal to extras.gaussian_fill.classify_cells + emit_points bit for bit.  counts: n_kept, n_shell, n_enclosed
    (cells).  One host read-back (the kept count sizes the output)."""
    field = field.reshape(-1)
    _gpu("field", field, torch.float32, ())
    o, h, d, dl = _lattice_args(origin, h, dims)
    nc = dl[0] * dl[1] * dl[2]
    if field.numel() != nc:
        raise ValueError(f"field of {field.numel()} cells does not match dims {dl}")
    n = int(per_cell)
    if n < 1:
        raise ValueError(f"per_cell must be >= 1, got {per_cell}")
    dev = field.device
    lib, stream = L.lib(), L.stream_ptr(dev)
    kind_cell = torch.empty(nc, dtype=torch.uint8, device=dev)
    offsets = torch.empty(nc, dtype=torch.int32, device=dev)
    cnt = torch.empty(3, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.nm_fill_classify_workspace(d)), 1), dtype=torch.uint8, device=dev)
    L.check(lib.nm_fill_classify(d, field.data_ptr(), float(density_thres), int(bool(include_shell)), kind_cell.data_ptr(),
                                 offsets.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream), "nm_fill_classify")
    n_kept, n_shell, n_enclosed = (int(v) for v in cnt.cpu())
    points = torch.empty((n_kept * n ** 3, 3), dtype=torch.float32, device=dev)
    kind = torch.empty(n_kept * n ** 3, dtype=torch.uint8, device=dev)
    L.check(lib.nm_fill_emit(d, o, h, n, int(bool(include_shell)), kind_cell.data_ptr(), offsets.data_ptr(), n_kept, points.data_ptr(),
                             kind.data_ptr(), stream), "nm_fill_emit")
    return points, kind, dict(n_kept=n_kept, n_shell=n_shell, n_enclosed=n_enclosed)


def fill_from_gaussians(means, cov6, opacity, resolution: int = 64, density_thres: float = 0.5, cutoff: float = 9.0,
                        per_cell: int = 1, include_shell: bool = True, device="cuda") -> Tuple[np.ndarray, np.ndarray, Dict]:
    """(points (M, 3) fp32, kind (M,) uint8: 1 shell / 2 enclosed, info) as numpy arrays: particles in the volume the activated
    Gaussians (`GaussianModel.get_xyz / get_covariance() / get_opacity`; tensors or arrays) describe.  `resolution` cells span
    the longest side of their bounding box; `cutoff` is the squared Mahalanobis radius beyond which a Gaussian contributes
    exactly 0; `per_cell`^3 particles per kept cell.  `density_thres` = 0.5 has not been chosen on a real capture.  info:
    dims, h, origin, n_shell, n_enclosed, n_skipped.  A non-GPU `device` runs extras.gaussian_fill (the same particles
    wherever no cell's density lies within rounding of the threshold).  Nothing to emit is a (0, 3) array, not an error;
    K = 0, non-finite inputs, more than 2^27 cells or more than 2^31 (Gaussian, block) pairs raise ValueError."""
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    mu, cv, op = cpu._inputs(as_np(means), as_np(cov6), as_np(opacity))
    dev = torch.device(device)
    if dev.type != "cuda":
        return cpu.fill_from_gaussians(mu, cv, op, resolution, density_thres, cutoff, per_cell, include_shell)
    if int(per_cell) < 1:
        raise ValueError(f"per_cell must be >= 1, got {per_cell}")
    origin, h, dims = cpu.fill_lattice(mu, cv, resolution, cutoff)
    dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    up = lambda a: (a.to(dev, torch.float32) if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(dev)).detach().contiguous()
    field, skipped = density_field(up(mu), up(cv), up(op), origin, h, dims, cutoff)
    points, kind, cnt = classify_emit(field, origin, h, dims, density_thres, per_cell, include_shell)
    info = dict(dims=tuple(int(d) for d in dims), h=h, origin=origin, n_shell=cnt["n_shell"], n_enclosed=cnt["n_enclosed"],
                n_skipped=skipped)
    return points.cpu().numpy().reshape(-1, 3), kind.cpu().numpy(), info


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fill the volume a kernels.ply describes with particles (particles.ply).")
    p.add_argument("--kernels", "-k", type=str, required=True, help="the Gaussians (kernels.ply / point_cloud.ply)")
    p.add_argument("--output", "-o", type=str, required=True, help="the particles.ply to write")
    p.add_argument("--sh_degree", type=int, default=3)
    p.add_argument("--resolution", type=int, default=64, help="lattice cells along the longest side")
    p.add_argument("--density_thres", type=float, default=0.5, help="shell threshold (default not tuned on a real capture)")
    p.add_argument("--cutoff", type=float, default=9.0, help="squared Mahalanobis radius of a Gaussian's support")
    p.add_argument("--per_cell", type=int, default=1, help="particles per kept cell and axis")
    p.add_argument("--no_shell", action="store_true", help="emit the enclosed cells only")
    p.add_argument("--opacity_thres", type=float, default=0.02, help="Gaussians at or below this opacity are ignored")
    p.add_argument("--device", type=str, default="cuda")
    return p.parse_args(argv)


@torch.no_grad()
def main(argv=None):
    from . import io as nio
    args = parse_args(argv)
    g = nio.load_gaussians_ply(args.kernels, args.sh_degree, device=args.device)
    keep = g.get_opacity.squeeze(-1) > args.opacity_thres
    print(f"Gaussians after pruning low opacity kernels: {int(keep.sum())} of {int(keep.numel())}")
    points, kind, info = fill_from_gaussians(g.get_xyz[keep], g.get_covariance()[keep], g.get_opacity.squeeze(-1)[keep],
                                             resolution=args.resolution, density_thres=args.density_thres, cutoff=args.cutoff,
                                             per_cell=args.per_cell, include_shell=not args.no_shell, device=args.device)
    nio.save_particles_ply(args.output, points)
    print(f"lattice {info['dims']}, h = {info['h']:.6g}: {info['n_shell']} shell and {info['n_enclosed']} enclosed cells, "
          f"{info['n_skipped']} degenerate Gaussians skipped -> {len(points)} particles in [{args.output}]")


if __name__ == "__main__":
    sys.exit(main())
