"""Triangle meshes out of a lattice field, in numpy fp64: the CPU path of neuma_amd/surface_mesh.py and the yardstick its HIP
kernels (csrc/nm_surface.hip) are held to.  Nothing in the reference does this.

Marching tetrahedra on the Kuhn subdivision, not marching cubes: six tetrahedra per cube need no 256-case table and have no
ambiguous case, and the result is the exact level set of a piecewise-linear interpolant, hence a closed 2-manifold.  The
algorithm, stated once for both paths:
    samples    `field` (n0 n1 n2,) in the layout of nm_fill_density: linear index (ix n1 + iy) n2 + iz, sample i at
               origin + (i + 1/2) h.  The lattice is extended by one ring of virtual samples of value 0 on every side
               (extended dims E = n + 2, extended sample e = i + 1, linear index (ex E1 + ey) E2 + ez), so that a body that
               touches the lattice's edge is still closed.  `iso` is finite and > 0 and taken as fp32.
    inside     f >= iso
    cubes      one per extended sample e, spanning e .. e + (1,1,1); the samples of the high faces own empty cubes.  Corner
               code = dx | dy << 1 | dz << 2.
    tetrahedra six per cube, in the order of PERMS: 000 -> e_p0 -> e_p0 + e_p1 -> 111.  The cut is the same in every cube,
               so face diagonals agree between neighbours.  A tetrahedron of an odd permutation is negatively oriented.
    edges      owned by their lower corner: 7 slots per sample, +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z (SLOT_CODE).  The mask
               of a sample has bit s set where the ends of slot s differ in the inside test - which also makes it the
               inside pattern of the sample's own cube relative to its corner 000.
    vertices   one per crossed edge, at p_a + t (p_b - p_a), t = (iso - f_a) / (f_b - f_a), a the OWNING corner whichever
               side it is on; numbered by owning sample (ascending extended linear index), then by slot.
    triangles  0, 1 or 2 per tetrahedron (tet_table), wound so that the normal points from inside to outside; ordered by
               cube (ascending), tetrahedron (PERMS order), then the tetrahedron's triangles.  A corner's index is
               offset[owner] + popcount(mask[owner] below its slot).  Zero-area triangles are KEPT: they appear when a
               sample equals iso exactly (t = 0 or 1 collapses an edge of the triangle), and dropping them would open the
               surface - topology comes before geometry here.
    normals    per vertex, the normalised negative gradient; the gradient is the central difference f(e + 1_a) - f(e - 1_a)
               at the two end samples (everything outside the real lattice is 0; the common factor 1 / (2 h) cancels),
               interpolated with the same t.  A zero gradient gives (0, 0, 0).
    attributes optional (A, ncells), A <= 4, interpolated along the edge with the same t; a ring sample carries the
               attribute of the nearest real sample.
`enclosed_volume` clips every tetrahedron in closed form and never looks at the triangle list: it is the independent check
of the triangles (divergence theorem, `mesh_volume`)."""
from typing import Dict, Optional, Tuple

import numpy as np

MAX_CELLS = 1 << 27
MAX_ATTRS = 4
_INT32_MAX = int(np.iinfo(np.int32).max)

SLOT_CODE = (1, 2, 4, 3, 6, 5, 7)             # slot -> corner code of the edge's far end
CODE_SLOT = (-1, 0, 1, 3, 2, 5, 4, 6)         # its inverse
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TET_CORNERS = tuple((0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in PERMS)
TET_ODD = (0, 1, 1, 0, 0, 1)                  # parity of the permutation = orientation of the tetrahedron
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _odd(seq) -> bool:
    return sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j]) % 2 == 1


def tet_table():
    """case (bit i = vertex i inside) -> triangles of a POSITIVELY oriented tetrahedron (v0, v1, v2, v3), each three indices
    into TET_EDGES, normal from inside to outside.  A negatively oriented tetrahedron swaps the last two indices.
      one vertex a apart from (b, c, d), det(b - a, c - a, d - a) > 0: (ab, ac, ad) has its normal away from a: the
          triangle when a alone is inside, reversed when a alone is outside
      a, b inside and c, d outside with (a, b, c, d) positively oriented: the planar quad ac, ad, bd, bc, cut along ac - bd"""
    e = {pair: i for i, pair in enumerate(TET_EDGES)}
    E = lambda i, j: e[(min(i, j), max(i, j))]
    table = []
    for case in range(16):
        ins = [i for i in range(4) if case >> i & 1]
        out = [i for i in range(4) if not case >> i & 1]
        if len(ins) in (1, 3):
            a = (ins if len(ins) == 1 else out)[0]
            b, c, d = [i for i in range(4) if i != a]
            if _odd((a, b, c, d)):
                c, d = d, c
            tri = (E(a, b), E(a, c), E(a, d))
            table.append((tri,) if len(ins) == 1 else ((tri[0], tri[2], tri[1]),))
        elif len(ins) == 2:
            (a, b), (c, d) = ins, out
            if _odd((a, b, c, d)):
                c, d = d, c
            table.append(((E(a, c), E(a, d), E(b, d)), (E(a, c), E(b, d), E(b, c))))
        else:
            table.append(())
    return tuple(table)


TET_TABLE = tet_table()


def _lattice(field, origin, h, dims, iso):
    d = tuple(int(x) for x in np.asarray(dims).reshape(3))
    if min(d) < 1 or d[0] * d[1] * d[2] > MAX_CELLS:
        raise ValueError(f"lattice dims {d} must be >= 1 and hold at most 2^27 cells")
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    if not (np.isfinite(o).all() and np.isfinite(h) and h > 0):
        raise ValueError("lattice origin / cell edge must be finite, the edge positive")
    iso = float(np.float32(iso))              # the native path takes it as fp32
    if not (np.isfinite(iso) and iso > 0):
        raise ValueError(f"iso must be finite and > 0, got {iso}")
    f = np.asarray(field).reshape(-1)
    if f.size != d[0] * d[1] * d[2]:
        raise ValueError(f"field of {f.size} cells does not match dims {d}")
    if not np.isfinite(f).all():
        raise ValueError("the field holds non-finite values")
    Fe = np.zeros(tuple(x + 2 for x in d), dtype=np.float64)
    Fe[1:-1, 1:-1, 1:-1] = f.reshape(d)
    return Fe, o, float(h), d, iso


def _shift(Ah, code):
    """The array of the far corner `code` for every extended sample; Ah is padded by one at the high end of every axis."""
    dx, dy, dz = code & 1, code >> 1 & 1, code >> 2 & 1
    n = [s - 1 for s in Ah.shape[:3]]
    return Ah[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]]


def _masks(Fe, iso):
    inside = Fe >= iso
    ih = np.pad(inside, ((0, 1),) * 3)
    mask = np.zeros(Fe.shape, dtype=np.uint8)
    for s, code in enumerate(SLOT_CODE):
        mask |= ((inside != _shift(ih, code)).astype(np.uint8) << s).astype(np.uint8)
    return inside, mask


def _cube_cases(inside_flat, mask_flat, cubes):
    """(n, 6) tetrahedron cases of the cubes `cubes` (extended linear indices)."""
    m = mask_flat[cubes].astype(np.int64)
    in0 = inside_flat[cubes].astype(np.int64)
    corner = [in0] + [in0 ^ (m >> CODE_SLOT[c] & 1) for c in range(1, 8)]
    return np.stack([sum(corner[TET_CORNERS[k][i]] << i for i in range(4)) for k in range(6)], 1)


def count(field, origin, h, dims, iso) -> Dict:
    """What nm_surface_count produces, over the extended lattice: mask (NE,) uint8, tri_count (NE,) uint8, their exclusive
    prefix sums vert_offset / tri_offset (NE,) int64 and the totals V, T."""
    Fe, o, h, d, iso = _lattice(field, origin, h, dims, iso)
    inside, mask = _masks(Fe, iso)
    mask_flat, inside_flat = mask.reshape(-1), inside.reshape(-1)
    cubes = np.flatnonzero(mask_flat)
    ntri = np.array([len(t) for t in TET_TABLE], dtype=np.int64)
    cases = _cube_cases(inside_flat, mask_flat, cubes)
    tri_count = np.zeros(mask_flat.size, dtype=np.uint8)
    tri_count[cubes] = ntri[cases].sum(1)
    vc = _POPCOUNT[mask_flat]
    voff = np.cumsum(vc) - vc
    tc = tri_count.astype(np.int64)
    toff = np.cumsum(tc) - tc
    V, T = int(vc.sum()), int(tc.sum())
    if V > _INT32_MAX or T > _INT32_MAX:
        raise ValueError(f"{V} vertices / {T} triangles do not fit an int32")
    return dict(mask=mask_flat, tri_count=tri_count, vert_offset=voff, tri_offset=toff, V=V, T=T, Fe=Fe, inside=inside_flat,
                cubes=cubes, cases=cases, origin=o, h=h, dims=d, iso=iso)


def _attrs(attrs, d):
    if attrs is None:
        return np.zeros((0,) + tuple(x + 3 for x in d), dtype=np.float64)
    a = np.asarray(attrs, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] > MAX_ATTRS or a.shape[1] != d[0] * d[1] * d[2]:
        raise ValueError(f"attrs must be (A <= {MAX_ATTRS}, {d[0] * d[1] * d[2]}), got {a.shape}")
    # ring: the nearest real sample; one more layer at the high end for the far-corner lookup (never used by a crossed edge)
    return np.pad(a.reshape((a.shape[0],) + d), ((0, 0),) + ((1, 2),) * 3, mode="edge")


def edge_crossings(field, origin, h, dims, iso) -> Dict:
    """The vertices as (owner (V,) extended linear index, slot (V,), t (V,), grad_a, grad_b (V, 3)) in their final order, on
    top of `count`'s result: what the tests of the native path derive their bounds from."""
    c = count(field, origin, h, dims, iso)
    Fe, E = c["Fe"], c["Fe"].shape
    bits = (c["mask"][:, None] >> np.arange(7)[None, :] & 1).astype(bool)
    owner, slot = np.nonzero(bits)                   # row-major: by sample, then by slot
    code = np.asarray(SLOT_CODE)[slot]
    ea = np.stack(np.unravel_index(owner, E), 1)
    eb = ea + np.stack([code & 1, code >> 1 & 1, code >> 2 & 1], 1)
    Fp = np.pad(Fe, 1)
    G = np.stack([Fp[2:, 1:-1, 1:-1] - Fp[:-2, 1:-1, 1:-1], Fp[1:-1, 2:, 1:-1] - Fp[1:-1, :-2, 1:-1],
                  Fp[1:-1, 1:-1, 2:] - Fp[1:-1, 1:-1, :-2]], -1)
    fa, fb = Fe[tuple(ea.T)], Fe[tuple(eb.T)]
    c.update(owner=owner, slot=slot, ea=ea, eb=eb, t=(c["iso"] - fa) / (fb - fa), grad_a=G[tuple(ea.T)], grad_b=G[tuple(eb.T)])
    return c


def extract(field, origin, h, dims, iso, attrs=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(vertices (V, 3), normals (V, 3), attrs (V, A), triangles (T, 3) int32) of the level set `iso` of `field`, fp64.  An
    empty surface gives arrays of length 0.  Zero-area triangles are kept (module docstring).  ValueError: non-finite field
    values, iso <= 0, more than 2^27 cells, V or T beyond int32."""
    c = edge_crossings(field, origin, h, dims, iso)
    o, h, d = c["origin"], c["h"], c["dims"]
    A = _attrs(attrs, d)
    t = c["t"][:, None]
    pa = o[None, :] + ((c["ea"] - 1).astype(np.float64) + 0.5) * h
    pb = o[None, :] + ((c["eb"] - 1).astype(np.float64) + 0.5) * h
    vertices = pa + t * (pb - pa)
    g = c["grad_a"] + t * (c["grad_b"] - c["grad_a"])
    norm = np.sqrt((g * g).sum(1, keepdims=True))
    normals = np.where(norm > 0, -g / np.where(norm > 0, norm, 1.0), 0.0)
    aa = A[(slice(None),) + tuple(c["ea"].T)].T
    ab = A[(slice(None),) + tuple(c["eb"].T)].T
    vattrs = aa + t * (ab - aa)

    E = c["Fe"].shape
    cubes, cases, mask, voff = c["cubes"], c["cases"], c["mask"].astype(np.int64), c["vert_offset"]
    ntri = np.array([len(x) for x in TET_TABLE], dtype=np.int64)
    per_tet = ntri[cases]                                               # (n, 6)
    start = c["tri_offset"][cubes][:, None] + np.cumsum(per_tet, 1) - per_tet
    flat_off = [(k & 1) * E[1] * E[2] + (k >> 1 & 1) * E[2] + (k >> 2 & 1) for k in range(8)]
    triangles = np.zeros((c["T"], 3), dtype=np.int32)
    for k in range(6):
        for case in range(1, 15):
            sel = np.flatnonzero(cases[:, k] == case)
            if sel.size == 0:
                continue
            for j, tri in enumerate(TET_TABLE[case]):
                tri = (tri[0], tri[2], tri[1]) if TET_ODD[k] else tri
                for q, edge in enumerate(tri):
                    ci, cj = (TET_CORNERS[k][v] for v in TET_EDGES[edge])
                    own = cubes[sel] + flat_off[ci]
                    s = CODE_SLOT[ci ^ cj]
                    triangles[start[sel, k] + j, q] = voff[own] + _POPCOUNT[mask[own] & ((1 << s) - 1)]
    return vertices, normals, vattrs, triangles


def mesh_volume(vertices, triangles) -> float:
    """Volume enclosed by a closed, outward oriented triangle mesh (divergence theorem), about the vertices' mean."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(triangles).reshape(-1, 3)
    if len(f) == 0:
        return 0.0
    p = v - v.mean(0)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


def enclosed_volume(field, origin, h, dims, iso) -> float:
    """Volume of {interpolant >= iso}: every tetrahedron clipped in closed form, from the samples alone (no triangle list).
    Tetrahedron volume W = h^3 / 6, u_ij = (iso - f_i) / (f_j - f_i) the crossing's fraction from i to j:
      a alone inside: W u_ab u_ac u_ad;  a alone outside: W (1 - u_ab u_ac u_ad)
      a, b inside: the prism (a, ac, ad | b, bc, bd), cut into three tetrahedra."""
    c = count(field, origin, h, dims, iso)
    h, iso, Fe, E = c["h"], c["iso"], c["Fe"], c["Fe"].shape
    inside, mask, cubes, cases = c["inside"], c["mask"], c["cubes"], c["cases"]
    ih = np.pad(inside.reshape(E), ((0, 1),) * 3)
    full = np.logical_and.reduce([_shift(ih, k) for k in range(8)])        # cubes wholly inside
    vol = float(full.sum()) * h ** 3
    Fh = np.pad(Fe, ((0, 1),) * 3)
    f8 = np.stack([_shift(Fh, k).reshape(-1)[cubes] for k in range(8)], 1)   # (n, 8) corner values
    W = h ** 3 / 6.0
    pos = np.array([[k & 1, k >> 1 & 1, k >> 2 & 1] for k in range(8)], dtype=np.float64)
    tetvol = lambda p0, p1, p2, p3: np.abs(np.einsum("ij,ij->i", p1 - p0, np.cross(p2 - p0, p3 - p0))) / 6.0
    for k in range(6):
        cs = TET_CORNERS[k]
        fv = f8[:, cs]                                                   # (n, 4)
        pv = pos[list(cs)]                                               # (4, 3) in units of h
        vol += float((cases[:, k] == 15).sum()) * W
        for case in range(1, 15):
            sel = np.flatnonzero(cases[:, k] == case)
            if sel.size == 0:
                continue
            ins = [i for i in range(4) if case >> i & 1]
            out = [i for i in range(4) if not case >> i & 1]
            u = lambda i, j: (iso - fv[sel, i]) / (fv[sel, j] - fv[sel, i])
            if len(ins) == 1:
                a = ins[0]
                vol += float(np.prod([u(a, j) for j in out], 0).sum()) * W
            elif len(ins) == 3:
                a = out[0]
                vol += float((1.0 - np.prod([u(a, j) for j in ins], 0)).sum()) * W
            else:
                (a, b), (cc, dd) = ins, out
                P = lambda i, j: pv[i][None, :] + u(i, j)[:, None] * (pv[j] - pv[i])[None, :]
                A0 = np.broadcast_to(pv[a], (sel.size, 3))
                B0 = np.broadcast_to(pv[b], (sel.size, 3))
                A1, A2, B1, B2 = P(a, cc), P(a, dd), P(b, cc), P(b, dd)
                vol += float((tetvol(A0, A1, A2, B0) + tetvol(A1, A2, B0, B1) + tetvol(A2, B0, B1, B2)).sum()) * h ** 3
    return vol


def mesh_topology(triangles, n_vertices: int) -> Dict:
    """Integer facts about a triangle list: closed (every undirected edge in exactly two triangles), oriented (the two
    traverse it in opposite directions), indices in range, every vertex used, and V, E, F with the Euler number."""
    f = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = int(n_vertices)
    if len(f) == 0:
        return dict(closed=True, oriented=True, in_range=True, all_used=V == 0, V=V, E=0, F=0, euler=V)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    in_range = bool(f.min() >= 0 and f.max() < V)
    key_d = a * (V + 1) + b
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, cnt = np.unique(lo * (V + 1) + hi, return_counts=True)
    closed = bool((cnt == 2).all()) and bool((a != b).all())
    # oriented: no directed edge twice (with closedness: each undirected edge once in each direction)
    oriented = closed and len(np.unique(key_d)) == len(key_d)
    used = np.zeros(V, dtype=bool)
    if in_range:
        used[f.reshape(-1)] = True
    return dict(closed=closed, oriented=oriented, in_range=in_range, all_used=bool(used.all()), V=V, E=int(len(cnt)), F=int(len(f)),
                euler=V - int(len(cnt)) + int(len(f)))
