"""Roll-outs as triangle meshes: the level set of the Gaussians' opacity density as a closed, consistently oriented, indexed
mesh - the one form a DCC tool, a game engine, a slicer or another simulator takes, and what `mesh_inside`, `mesh_sdf` and the
mesh colliders take back (a frame of one roll-out becomes a collider or a body of the next).  No reference counterpart.
extras/surface_mesh.py states the algorithm (marching tetrahedra on the Kuhn subdivision of the lattice, extended by one ring of
zero samples) and is the CPU path; here it runs as HIP kernels (csrc/nm_surface.hip): one counting pass, two prefix sums, one
emission pass that writes every vertex and triangle to its final slot - no hash, no sort, no welding, integer sums only, so two
runs give identical bytes and the connectivity equals the numpy path's exactly.

    python -m neuma_amd.surface_mesh (-s GAUSSIANS_DIR | -k kernels.ply) -o OUT [--resolution R] [--density_thres T]
        [--cutoff C] [--no_colors] [--sh_degree D] [--format ply|obj] [--opacity_thres 0.0] [--device cuda]

-k turns one 3DGS file into the mesh OUT; -s turns every NNN.ply of a folder (`render --save_gaussians`, `inference
--save_gaussians`, or the painted gaussians_NAME_<quantity>/ of --color_by, read with --sh_degree 0) into OUT/NNN.ply: a mesh
sequence with the same names.  Needs no simulator, checkpoints or bindings.  One line per frame: V, T and the enclosed volume
(divergence theorem).  `density_thres` = 0.5 is a default nobody has tuned on a real capture yet."""
import argparse
import sys
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .extras import gaussian_fill as fill_cpu
from .extras import surface_mesh as cpu
from .gaussian_fill import _gpu, _lattice_args, density_field
from .render.general_utils import C0


def _iso(iso) -> float:
    v = float(np.float32(iso))            # the kernels take it as fp32
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"iso must be finite and > 0, got {iso}")
    return v


def count(field: torch.Tensor, dims, iso) -> Dict:
    """nm_surface_count on a device field (ncells,) fp32: mask, tri_count (NE,) uint8 and vert_offset, tri_offset (NE,) int32
    over the extended lattice (dims + 2), and the totals V, T.  One host read-back (the totals and the non-finite flag).
    ValueError: a non-finite field value, V or T beyond int32."""
    field = field.reshape(-1)
    _gpu("field", field, torch.float32, ())
    _, _, d, dl = _lattice_args((0.0, 0.0, 0.0), 1.0, dims)
    if field.numel() != dl[0] * dl[1] * dl[2]:
        raise ValueError(f"field of {field.numel()} cells does not match dims {dl}")
    iso = _iso(iso)
    dev = field.device
    lib, stream = L.lib(), L.stream_ptr(dev)
    ne = (dl[0] + 2) * (dl[1] + 2) * (dl[2] + 2)
    mask = torch.empty(ne, dtype=torch.uint8, device=dev)
    tri_count = torch.empty(ne, dtype=torch.uint8, device=dev)
    voff = torch.empty(ne, dtype=torch.int32, device=dev)
    toff = torch.empty(ne, dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.nm_surface_workspace(d))
    if ws_bytes == 0:
        raise L.NeumaHipError(f"nm_surface_workspace rejects dims {dl}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    L.check(lib.nm_surface_count(d, field.data_ptr(), iso, mask.data_ptr(), tri_count.data_ptr(), voff.data_ptr(), toff.data_ptr(),
                                 info.data_ptr(), ws.data_ptr(), ws.numel(), stream), "nm_surface_count")
    V, T, bad = (int(v) for v in info.cpu())
    if bad:
        raise ValueError("the field holds non-finite values")
    if V > np.iinfo(np.int32).max or T > np.iinfo(np.int32).max:
        raise ValueError(f"{V} vertices / {T} triangles do not fit an int32")
    return dict(mask=mask, tri_count=tri_count, vert_offset=voff, tri_offset=toff, V=V, T=T)


def extract(field: torch.Tensor, origin, h, dims, iso, attrs: Optional[torch.Tensor] = None, return_count: bool = False):
    """(vertices (V, 3) fp32, normals (V, 3) fp32, attrs (V, A) fp32, triangles (T, 3) int32) of the level set `iso` of `field`
    (ncells,) fp32 in the layout of `density_field`, sample i at origin + (i + 1/2) h; `attrs` (A <= 4, ncells) fp32 is
    interpolated onto the vertices.  Device tensors in, device tensors out, one host read-back (the totals size the outputs).
    The mesh is closed and oriented outwards (from f >= iso to f < iso) on any finite field; zero-area triangles are kept
    (extras/surface_mesh.py).  An empty surface gives tensors of length 0.  A CPU `field` takes the extras path (fp64 inside,
    the same dtypes out).  ValueError: non-finite field values, iso <= 0, more than 2^27 cells, V or T beyond int32.  With
    `return_count` the result of `count` (device tensors; the extras path's arrays for a CPU field) is appended."""
    if not field.is_cuda:
        a = None if attrs is None else attrs.detach().cpu().numpy()
        v, n, va, tri = cpu.extract(field.detach().cpu().numpy(), origin, h, dims, iso, a)
        out = (torch.from_numpy(v.astype(np.float32)), torch.from_numpy(n.astype(np.float32)), torch.from_numpy(va.astype(np.float32)),
               torch.from_numpy(tri))
        return out + (cpu.count(field.detach().cpu().numpy(), origin, h, dims, iso),) if return_count else out
    field = field.reshape(-1)
    o, h, d, dl = _lattice_args(origin, h, dims)
    nc = dl[0] * dl[1] * dl[2]
    A = 0
    if attrs is not None:
        attrs = attrs.reshape(1, -1) if attrs.dim() == 1 else attrs
        _gpu("attrs", attrs, torch.float32, (nc,))
        A = int(attrs.shape[0])
        if A > cpu.MAX_ATTRS:
            raise ValueError(f"at most {cpu.MAX_ATTRS} attributes, got {A}")
        L.same_device(field, attrs)
    c = count(field, dl, iso)
    dev = field.device
    V, T = c["V"], c["T"]
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    vattrs = torch.empty((V, A), dtype=torch.float32, device=dev)
    tris = torch.empty((T, 3), dtype=torch.int32, device=dev)
    L.check(L.lib().nm_surface_emit(d, o, h, field.data_ptr(), _iso(iso), A, attrs.data_ptr() if A else None, c["mask"].data_ptr(),
                                    c["tri_count"].data_ptr(), c["vert_offset"].data_ptr(), c["tri_offset"].data_ptr(), V, T,
                                    verts.data_ptr(), normals.data_ptr(), vattrs.data_ptr() if A else None, tris.data_ptr(),
                                    L.stream_ptr(dev)), "nm_surface_emit")
    out = (verts, normals, vattrs, tris)
    return out + (c,) if return_count else out


@torch.no_grad()
def surface_from_gaussians(model, resolution: int = 128, density_thres: float = 0.5, cutoff: float = 9.0, colors: bool = True,
                           opacity_thres: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor, Dict]:
    """(vertices (V, 3), normals (V, 3), colors (V, 3) in [0, 1] or None, triangles (T, 3) int32, info) on the model's device:
    the surface {density = density_thres} of a GaussianModel's opacity density, on the lattice of
    extras.gaussian_fill.fill_lattice (`resolution` cells along the longest side, `cutoff` the squared Mahalanobis radius of a
    Gaussian's support).  With `colors` a vertex carries the opacity-weighted mean of rgb = clamp(1/2 + C0 f_dc, 0, 1) of the
    Gaussians around it (three more density fields with weight opacity * rgb, divided by the density; 0 where it is 0).
    Gaussians at or below `opacity_thres` are left out.  `density_thres` = 0.5 has not been chosen on a real capture.  info:
    origin, h, dims, iso, n_skipped, field (the density, on the device).  A model on the CPU takes the extras path."""
    keep = model.get_opacity.detach().reshape(-1) > float(opacity_thres)
    means = model.get_xyz.detach()[keep].float().contiguous()
    cov6 = model.get_covariance().detach()[keep].float().contiguous()
    opacity = model.get_opacity.detach().reshape(-1)[keep].float().contiguous()
    rgb = (0.5 + C0 * model._features_dc.detach().reshape(-1, 3)[keep].float()).clamp(0.0, 1.0)
    mu, cv, op = fill_cpu._inputs(means.cpu().numpy(), cov6.cpu().numpy(), opacity.cpu().numpy())
    origin, h, dims = fill_cpu.fill_lattice(mu, cv, resolution, cutoff)
    iso = _iso(density_thres)
    if means.is_cuda:
        fields = lambda w: density_field(means, cov6, w.contiguous(), origin, h, dims, cutoff)
    else:
        def fields(w):
            f, skipped = fill_cpu.density_field(mu, cv, w.numpy(), origin, h, dims, cutoff)
            return torch.from_numpy(f.astype(np.float32)), skipped
    field, skipped = fields(opacity)
    attrs = None
    if colors:
        num = torch.stack([fields(opacity * rgb[:, c])[0] for c in range(3)], 0)
        attrs = torch.where(field[None, :] > 0, num / field[None, :].clamp_min(1e-38), torch.zeros_like(num)).contiguous()
    verts, normals, vcol, tris = extract(field, origin, h, dims, iso, attrs)
    info = dict(origin=origin, h=h, dims=tuple(int(d) for d in dims), iso=iso, n_skipped=skipped, field=field)
    return verts, normals, (vcol.clamp(0.0, 1.0) if colors else None), tris, info


def save_surface(path, model, resolution: int = 128, density_thres: float = 0.5, cutoff: float = 9.0, colors: bool = True,
                 opacity_thres: float = 0.0, fmt: str = "ply") -> Dict:
    """surface_from_gaussians(model) written to `path` (io.save_mesh_ply / io.save_mesh_obj); returns V, T, volume (divergence
    theorem, fp64) and the lattice dims."""
    from . import io as nio
    v, n, c, t, info = surface_from_gaussians(model, resolution, density_thres, cutoff, colors, opacity_thres)
    v, n, t = v.cpu().numpy(), n.cpu().numpy(), t.cpu().numpy()
    c = None if c is None else c.cpu().numpy()
    (nio.save_mesh_obj if fmt == "obj" else nio.save_mesh_ply)(path, v, n, c, t)
    return dict(V=len(v), T=len(t), volume=cpu.mesh_volume(v, t), dims=info["dims"])


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Turn 3DGS files (one, or the NNN.ply frames of a folder) into closed triangle meshes.")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--source", "-s", type=str, help="folder of NNN.ply Gaussian frames (--save_gaussians): one mesh per frame")
    src.add_argument("--kernels", "-k", type=str, help="one 3DGS file (kernels.ply / point_cloud.ply)")
    p.add_argument("--output", "-o", type=str, required=True, help="the mesh file (-k) or the folder of NNN meshes (-s)")
    p.add_argument("--resolution", type=int, default=128, help="lattice cells along the longest side")
    p.add_argument("--density_thres", type=float, default=0.5, help="level of the surface (default not tuned on a real capture)")
    p.add_argument("--cutoff", type=float, default=9.0, help="squared Mahalanobis radius of a Gaussian's support")
    p.add_argument("--no_colors", action="store_true", help="write no vertex colours")
    p.add_argument("--sh_degree", type=int, default=3, help="must match the files' f_rest_* count (0 for painted frames)")
    p.add_argument("--format", type=str, default="ply", choices=("ply", "obj"))
    p.add_argument("--opacity_thres", type=float, default=0.0, help="Gaussians at or below this opacity are ignored")
    p.add_argument("--device", type=str, default="cuda")
    return p.parse_args(argv)


@torch.no_grad()
def main(argv=None):
    from . import io as nio
    args = parse_args(argv)
    if args.kernels is not None:
        jobs = [(Path(args.kernels), Path(args.output))]
    else:
        out = Path(args.output)
        out.mkdir(parents=True, exist_ok=True)
        frames = sorted((p for p in Path(args.source).glob("*.ply") if p.stem.isdigit()), key=lambda p: int(p.stem))
        if not frames:
            raise FileNotFoundError(f"no NNN.ply frames in {args.source}")
        jobs = [(p, out / f"{p.stem}.{args.format}") for p in frames]
    for src, dst in jobs:
        g = nio.load_gaussians_ply(src, args.sh_degree, device=args.device)
        r = save_surface(dst, g, args.resolution, args.density_thres, args.cutoff, not args.no_colors, args.opacity_thres, args.format)
        print(f"{src.name}: lattice {r['dims']}, V = {r['V']}, T = {r['T']}, volume = {r['volume']:.6g} -> [{dst}]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
