"""Signed distance field of a closed triangle mesh on a regular lattice, in numpy: the DEFINITION the native kernel
(csrc/nm_sdf.hip, nm_mesh_distance) is held to, and the CPU path of neuma_amd.mesh_sdf.  No reference counterpart.

Lattice: node (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing; arrays are (nx, ny, nz), ix-major.  `origin` and `spacing`
are fp32 values (the C ABI takes floats); the vertices are rounded to fp32 first for the same reason.

Distance to one triangle (a, b, c) - closest point by Voronoi region, every operation in the dtype asked for (fp64: the
yardstick; fp32: the same operations in the same order as the kernel, which is built without fma contraction):

    ab = b - a, ac = c - a, aa = ab.ab, bb = ab.ac, cc = ac.ac                  (the triangle's record)
    ap = p - a, d1 = ab.ap, d2 = ac.ap, d3 = d1 - aa, d4 = d2 - bb, d5 = d1 - bb, d6 = d2 - cc
    va = d3 d6 - d5 d4, vb = d5 d2 - d1 d6, vc = d1 d4 - d3 d2
    region (first that holds)                           nv        nw        den
      vertex a   d1 <= 0, d2 <= 0                       0         0         1
      vertex b   d3 >= 0, d4 <= d3                      1         0         1
      edge ab    vc <= 0, d1 >= 0, d3 <= 0              d1        0         d1 - d3
      vertex c   d6 >= 0, d5 <= d6                      0         1         1
      edge ac    vb <= 0, d2 >= 0, d6 <= 0              0         d2        d2 - d6
      edge bc    va <= 0, d4 - d3 >= 0, d5 - d6 >= 0    d5 - d6   d4 - d3   (d4 - d3) + (d5 - d6)
      face                                              vb        vc        (va + vb) + vc
    r = 1 / den, v = nv r, w = nw r, e = (ab v + ac w) - ap, dist^2 = e.e

A dot product is (x0 y0 + x1 y1) + x2 y2.  A DEGENERATE triangle - aa cc - bb bb not above DEGENERATE_REL aa cc - takes the
minimum over its three edge segments instead (q0 + t e, t = clamp((e.(p - q0)) / (e.e), 0, 1); t = 0 on a zero-length
segment).  The field is sqrt(min over the kept triangles of dist^2), +inf without one; a triangle with a vertex index outside
[0, n_verts) is dropped.  Vertices are expected to be finite.

build_mesh_field turns that into the signed field of a closed mesh: the sign comes from extras.mesh_sampling.points_in_mesh
(ray parity in fp64) at the nodes.  Not on the frame path; imports nothing from the test oracle.
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import mesh_sampling as ms

DEGENERATE_REL = 1e-6      # sin^2 of the angle at a: below it fp32 no longer resolves aa cc - bb bb (its rounding is ~1e-7 aa cc)
MAX_NODES = 1 << 27
MAX_TRIS = 1 << 24


@dataclass
class MeshField:
    """phi (nx, ny, nz): signed distance at the lattice nodes (negative inside), a numpy array (CPU path) or a torch tensor
    on the device (GPU path); origin (3,) and spacing as the fp32 values both paths computed with; dims (nx, ny, nz)."""
    phi: object
    origin: Tuple[float, float, float]
    spacing: float
    dims: Tuple[int, int, int]


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def kept_triangles(n_verts: int, tris) -> np.ndarray:
    """(m, 3) int64: the triangles whose three vertex indices lie in [0, n_verts)."""
    t = np.asarray(tris)
    t = t.reshape(-1, 3).astype(np.int64) if t.size else np.zeros((0, 3), dtype=np.int64)
    return t[((t >= 0) & (t < int(n_verts))).all(axis=1)]


def triangle_records(verts, tris, dtype=np.float64):
    """(a, ab, ac, aa, bb, cc) of the kept triangles, computed in `dtype` from the fp32 vertices."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(dtype)
    t = kept_triangles(len(v), tris)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac = b - a, c - a
    return a, ab, ac, _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)


def _segment_dist2(q0, e, p):
    ep = p - q0
    ee = _dot(e, e)
    one, zero = ee.dtype.type(1), ee.dtype.type(0)
    t = _dot(e, ep) / np.where(ee > zero, ee, one)
    t = np.minimum(np.maximum(t, zero), one)
    d = ep - e * t[..., None]
    return _dot(d, d)


def pair_dist2(p, rec):
    """Squared distances of the points p (M, 3) to the triangles of `rec`: (M, T), in the records' dtype."""
    a, ab, ac, aa, bb, cc = (x[None] for x in rec)
    dt = rec[0].dtype
    one, zero = dt.type(1), dt.type(0)
    p = np.asarray(p, dtype=dt)[:, None, :]
    ap = p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4, d5, d6 = d1 - aa, d2 - bb, d1 - bb, d2 - cc
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    e43, e56 = d4 - d3, d5 - d6
    ones, zeros = np.full_like(d1, one), np.zeros_like(d1)
    nv, nw, den = vb, vc, (va + vb) + vc
    # the table bottom-up: a later np.where overrides, so the first region that holds wins
    for m, rv, rw, rd in (((va <= zero) & (e43 >= zero) & (e56 >= zero), e56, e43, e43 + e56),
                          ((vb <= zero) & (d2 >= zero) & (d6 <= zero), zeros, d2, d2 - d6),
                          ((d6 >= zero) & (d5 <= d6), zeros, ones, ones),
                          ((vc <= zero) & (d1 >= zero) & (d3 <= zero), d1, zeros, d1 - d3),
                          ((d3 >= zero) & (d4 <= d3), ones, zeros, ones),
                          ((d1 <= zero) & (d2 <= zero), zeros, zeros, ones)):
        nv, nw, den = np.where(m, rv, nv), np.where(m, rw, nw), np.where(m, rd, den)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = one / den
        v, w = nv * r, nw * r
        e = (ab * v[..., None] + ac * w[..., None]) - ap
        out = _dot(e, e)
    degenerate = ~(aa * cc - bb * bb > dt.type(DEGENERATE_REL) * (aa * cc))[0]
    if degenerate.any():
        a_, ab_, ac_ = a[:, degenerate], ab[:, degenerate], ac[:, degenerate]
        s = np.minimum(np.minimum(_segment_dist2(a_, ab_, p), _segment_dist2(a_, ac_, p)), _segment_dist2(a_ + ab_, ac_ - ab_, p))
        out[:, degenerate] = s
    return out


def lattice_nodes(origin, spacing, dims, dtype=np.float64) -> np.ndarray:
    """(nx, ny, nz, 3) node positions origin + index * spacing, evaluated in `dtype` from the fp32 origin and spacing."""
    o = np.asarray(origin, dtype=np.float32).astype(dtype)
    h = np.float32(spacing).astype(dtype)
    axes = [o[k] + np.arange(int(dims[k])).astype(dtype) * h for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


def check_lattice(spacing, dims) -> Tuple[int, int, int]:
    d = tuple(int(x) for x in dims)
    if len(d) != 3 or min(d) < 2:
        raise ValueError(f"dims: three lattice sizes >= 2 expected, got {dims!r}")
    if d[0] * d[1] * d[2] > MAX_NODES:
        raise ValueError(f"dims: {d[0]} x {d[1]} x {d[2]} nodes exceed 2^27")
    if not (np.isfinite(np.float32(spacing)) and np.float32(spacing) > 0):
        raise ValueError(f"spacing: must be positive and finite (got {spacing})")
    return d


def mesh_distance(verts, tris, origin, spacing, dims, dtype=np.float64, chunk: int = 2048) -> np.ndarray:
    """(nx, ny, nz) unsigned distance of every lattice node to the mesh, evaluated in `dtype` (module docstring)."""
    d = check_lattice(spacing, dims)
    dt = np.dtype(dtype)
    rec = triangle_records(verts, tris, dt)
    p = lattice_nodes(origin, spacing, d, dt).reshape(-1, 3)
    best = np.full(len(p), np.inf, dtype=dt)
    if len(rec[0]):
        step = max(1, int(chunk * 256 // max(len(rec[0]), 256)))
        for i0 in range(0, len(p), step):
            best[i0:i0 + step] = pair_dist2(p[i0:i0 + step], rec).min(axis=1)
    return np.sqrt(best).reshape(d)


def open_edges(n_verts: int, tris) -> int:
    """Number of undirected edges NOT shared by exactly two kept triangles (0: the mesh is closed)."""
    t = kept_triangles(n_verts, tris)
    if len(t) == 0:
        return 0
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return int((counts != 2).sum())


def check_closed_mesh(verts, tris) -> np.ndarray:
    """The kept triangles of a closed, outward-oriented mesh, or ValueError (open: the count of offending edges; `inverted`: a
    mesh_volume that is not positive)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = kept_triangles(len(v), tris)
    if len(t) == 0:
        raise ValueError("mesh is not closed: it has no triangle")
    bad = open_edges(len(v), t)
    if bad:
        raise ValueError(f"mesh is not closed: {bad} edges are not shared by exactly two triangles")
    vol = ms.mesh_volume(v, t)
    if not vol > 0.0:
        raise ValueError(f"mesh is inverted or flat: mesh_volume = {vol} is not positive (triangles must wind counter-clockwise "
                         "seen from outside)")
    return t


def field_lattice(verts, spacing=None, resolution: int = 64, margin_cells: int = 2):
    """(origin (3,) fp32, spacing fp32, dims): the mesh's bounding box grown by `margin_cells` cells on every side; `resolution`
    cells along the longest axis when `spacing` is None."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    if len(v) == 0 or not np.isfinite(v).all():
        raise ValueError("verts: finite vertices expected")
    lo, hi = v.min(0), v.max(0)
    m = int(margin_cells)
    if m < 0:
        raise ValueError(f"margin_cells: must not be negative (got {margin_cells})")
    if spacing is None:
        if int(resolution) < 1:
            raise ValueError(f"resolution: must be >= 1 (got {resolution})")
        spacing = float((hi - lo).max()) / int(resolution)
    h = np.float32(spacing)
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"spacing: must be positive and finite (got {spacing})")
    origin = (lo - m * float(h)).astype(np.float32)
    cells = np.ceil((hi - origin.astype(np.float64)) / float(h) - 1e-9).astype(np.int64)      # cells that reach hi from the origin
    dims = tuple(int(max(c, 1)) + m + 1 for c in cells)
    return origin, h, check_lattice(h, dims)


def signed_field(dist, inside):
    return np.where(inside, -dist, dist)


def build_mesh_field(verts, tris, spacing=None, resolution: int = 64, margin_cells: int = 2, dtype=np.float64) -> MeshField:
    """The signed distance field of a closed mesh on the CPU: |phi| = mesh_distance in `dtype`, phi < 0 exactly at the nodes
    extras.mesh_sampling.points_in_mesh calls inside."""
    t = check_closed_mesh(verts, tris)
    origin, h, dims = field_lattice(verts, spacing, resolution, margin_cells)
    dist = mesh_distance(verts, t, origin, h, dims, dtype)
    v64 = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    inside = ms.points_in_mesh(lattice_nodes(origin, h, dims).reshape(-1, 3), v64, t).reshape(dims)
    return MeshField(signed_field(dist, inside), tuple(float(x) for x in origin), float(h), dims)


def cull_order(n_tris: int) -> np.ndarray:
    """The order in which neuma_amd.mesh_sdf uploads the triangles: a fixed pseudo-random permutation.  The distance field does not
    depend on the order; the kernel's bounding-sphere cull does.  A wave skips a record only once its lanes hold a best distance
    smaller than the record's lower bound, so what pays is a tight bound EARLY: a random sample of the whole surface gives every
    block of nodes one within the first records.  A spatially sorted order (Morton code of the centroids, or a mesh generator's
    own) meets most blocks' near triangles late and measured 1.3 x slower ("Mesh colliders")."""
    return np.random.default_rng(0x5DF).permutation(int(n_tris))
