"""Meshes and lattices of the mesh-distance / mesh-collider tests, generated here (nothing is read from disk).  Every closed
mesh winds counter-clockwise seen from outside (positive mesh_volume)."""
import functools
import math

import numpy as np

LATTICE_DIMS = ((13, 9, 6), (33, 32, 17))      # neither is a multiple of 4 on every axis
BAD_DEPTH = 2e-6                               # how far under the surface the degenerate triangle of sphere320_bad lies


def icosahedron(radius=0.3, center=(0.5, 0.45, 0.55)):
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], dtype=np.float64)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], dtype=np.int64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v * radius + np.asarray(center), t


def subdivide(verts, tris, radius, center):
    """One 1 -> 4 split with the new vertices pushed back onto the sphere."""
    verts = [tuple(p) for p in verts]
    mid = {}

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            m = (np.asarray(verts[i]) + np.asarray(verts[j])) / 2.0 - np.asarray(center)
            verts.append(tuple(m / np.linalg.norm(m) * radius + np.asarray(center)))
            mid[key] = len(verts) - 1
        return mid[key]

    out = []
    for a, b, c in tris:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.asarray(verts, dtype=np.float64), np.asarray(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _sphere(level, radius=0.3, center=(0.5, 0.45, 0.55)):
    v, t = icosahedron(radius, center)
    for _ in range(level):
        v, t = subdivide(v, t, radius, center)
    return v, t


def sphere320():
    v, t = _sphere(2)
    return v.copy(), t.copy()


def torus(nu=16, nv=8, R=0.22, r=0.08, center=(0.5, 0.4, 0.5)):
    """nu x nv quads, two triangles each; the axis of the torus is y."""
    verts, tris = [], []
    for i in range(nu):
        a = 2 * math.pi * i / nu
        for j in range(nv):
            b = 2 * math.pi * j / nv
            rr = R + r * math.cos(b)
            verts.append((rr * math.cos(a), r * math.sin(b), rr * math.sin(a)))
    for i in range(nu):
        for j in range(nv):
            p00, p10 = i * nv + j, ((i + 1) % nu) * nv + j
            p01, p11 = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            tris += [(p00, p11, p10), (p00, p01, p11)]
    v, t = np.asarray(verts, dtype=np.float64) + np.asarray(center), np.asarray(tris, dtype=np.int64)
    return v, _outward(v, t)


def rotated_box(half=(0.2, 0.07, 0.15), euler_deg=(20.0, 35.0, 10.0), center=(0.5, 0.3, 0.5)):
    a, b, c = (math.radians(x) for x in euler_deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    corners = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * np.asarray(half)
    t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], dtype=np.int64)
    v = corners @ (Rz @ Ry @ Rx).T + np.asarray(center)
    return v, _outward(v, t)


def _outward(v, t):
    """flip the whole mesh when its signed volume is negative"""
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    return t if vol > 0 else t[:, ::-1].copy()


def sphere320_with_bad_triangles():
    """sphere320 plus one degenerate triangle and one triangle with an out-of-range index.  The degenerate one is three collinear
    points (two of them equal: one of its segments has zero length) on a short segment inside the sphere, BAD_DEPTH under the
    centroid of face 0 and parallel to it.  A node is nearer to that segment than to the surface only inside a needle of radius
    ~ sqrt(2 depth BAD_DEPTH) around the inward normal there; tests/test_mesh_sdf_cpu.py asserts that no node of the test
    lattices is, in fp64 and in fp32."""
    v, t = sphere320()
    n = len(v)
    a, b, c = v[t[0, 0]], v[t[0, 1]], v[t[0, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm)
    q = (a + b + c) / 3.0 - BAD_DEPTH * nrm
    e = (b - a) * 0.1
    extra = np.stack([q, q + e, q + e])
    v = np.concatenate([v, extra])
    t = np.concatenate([t, np.array([(n, n + 1, n + 2), (0, 1, n + 3)], dtype=np.int64)])
    return v, t


def many_triangles(n=257):
    """n triangles: the sphere's 320 cut to n (one more than an LDS tile of 256)"""
    v, t = sphere320()
    return v, t[:n]


def single_triangle():
    v = np.array([(0.31, 0.22, 0.4), (0.72, 0.35, 0.48), (0.45, 0.68, 0.61)], dtype=np.float64)
    return v, np.array([(0, 1, 2)], dtype=np.int64)


MESHES = {"icosahedron": lambda: icosahedron(), "sphere320": sphere320, "torus": lambda: torus(), "box": lambda: rotated_box(),
          "sphere320_bad": sphere320_with_bad_triangles, "tris257": many_triangles, "single": single_triangle}


def lattice_for(verts, dims, margin=0.06):
    """(origin fp32 (3,), spacing fp32) of a lattice of `dims` nodes that covers the mesh's box with a margin, cubic cells (the
    spacing of the tightest axis), deliberately not aligned with anything."""
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(0) - margin, v.max(0) + margin
    h = float(((hi - lo) / (np.asarray(dims) - 1)).max())
    return (lo + np.array([0.0013, 0.0007, 0.0021])).astype(np.float32), np.float32(h)


def write_obj(path, verts, tris):
    with open(path, "w") as f:
        for p in verts:
            f.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for a, b, c in tris:
            f.write(f"f {a + 1} {b + 1} {c + 1}\n")
