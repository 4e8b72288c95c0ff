"""Shared inputs of the driven-mesh tests (tests/test_mesh_drive_cpu.py, tests/test_gpu_mesh_drive.py), pure numpy: the smallest
meshes and particle clouds at which the bind, the frame product and the vertex normals can go wrong.  Every array is fp32 (the
values the kernels see); no vertex coordinate is -0.0, so "frame 0 is bitwise the input" can be asked of V0 + 0."""
import numpy as np

H = 1.0 / 12.0                  # lattice spacing of the jittered cloud


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32) + np.float32(0.0))


def icosphere(level: int):
    """(unit vertices (V, 3) fp64, triangles (T, 3) int32): V = 12, 42, 162, 642 for level 0 .. 3; outward orientation."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, dtype=np.int32)


def uv_sphere(segments: int = 100, rings: int = 5):
    """A UV sphere whose two poles have valence `segments`: V = 2 + segments rings."""
    v = [(0.0, 0.0, 1.0)]
    for r in range(1, rings + 1):
        th = np.pi * r / (rings + 1)
        for s in range(segments):
            ph = 2 * np.pi * s / segments
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda r, s: 1 + r * segments + s % segments
    f = [(0, ring(0, s), ring(0, s + 1)) for s in range(segments)]
    for r in range(rings - 1):
        for s in range(segments):
            f += [(ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)), (ring(r, s), ring(r + 1, s + 1), ring(r, s + 1))]
    last = len(v) - 1
    f += [(last, ring(rings - 1, s + 1), ring(rings - 1, s)) for s in range(segments)]
    return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int32)


def jittered_lattice(n: int = 12, seed: int = 0):
    """n^3 particles on the unit cube's cell centres, each moved by up to a quarter spacing: N = 1728 for n = 12."""
    rng = np.random.default_rng(seed)
    ax = (np.arange(n) + 0.5) / n
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return g + rng.uniform(-0.25, 0.25, g.shape) / n


def spiral_strip(n: int):
    """n unit vertices along a Fibonacci spiral and the triangle strip (i, i + 1, i + 2) over them: T = max(n - 2, 0)"""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / max(n, 1)
    ph = np.pi * (1.0 + 5.0 ** 0.5) * i
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], 1), np.asarray(_strip(n), dtype=np.int32).reshape(-1, 3)


def _strip(n: int):
    """the triangle strip over vertices 0 .. n-1, wound alike"""
    return [(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(max(n - 2, 0))]


def _case(V0, tri, X, ks=(16,), tie_free=True, degenerate=False, **extra):
    return dict(V0=_f32(V0), tri=np.ascontiguousarray(np.asarray(tri, dtype=np.int32).reshape(-1, 3)), X=_f32(X), ks=tuple(ks),
                tie_free=tie_free, degenerate=degenerate, **extra)


def all_cases():
    """name -> dict(V0 (V, 3) fp32, tri (T, 3) int32, X (N, 3) fp32, ks, tie_free, degenerate[, zero_normals, cancel])."""
    out = {}
    cloud = jittered_lattice()
    sv, st = icosphere(3)                                   # 642 vertices
    c = np.array([0.5, 0.5, 0.5])
    out["inside"] = _case(c + 0.3 * sv, st, cloud, ks=(8, 16))
    # the same lattice with the mesh half a spacing outside the cloud: every neighbourhood lies to one side of its vertex
    box = sv / np.abs(sv).max(1, keepdims=True)
    out["outside"] = _case(c + (0.5 + 0.5 * H) * box, st, cloud, ks=(8, 16))
    for n in (1, 63, 64, 65, 257):                          # one lane, either side of a wave, more than one workgroup
        v, t = spiral_strip(n)
        out[f"v{n}"] = _case(c + 0.3 * v, t, cloud, ks=(1, 4, 8, 16) if n == 65 else (16,))
    rng = np.random.default_rng(5)
    out["n_equals_k"] = _case(c + 0.2 * icosphere(0)[0], icosphere(0)[1], c + rng.uniform(-0.3, 0.3, (16, 3)), ks=(16,))
    # an exactly coplanar one-layer cloud (z = 1/2, jittered in the plane) under a vertex grid offset from it: rank-2 M
    ax = (np.arange(20) + 0.5) / 20
    sheet = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.01, 0.01, (400, 2))
    gx = 0.2 + 0.6 * np.arange(8) / 7
    gv = np.stack(np.meshgrid(gx, gx, indexing="ij"), -1).reshape(-1, 2)
    gi = lambda i, j: 8 * i + j
    gt = [q for i in range(7) for j in range(7) for q in ((gi(i, j), gi(i + 1, j), gi(i + 1, j + 1)), (gi(i, j), gi(i + 1, j + 1), gi(i, j + 1)))]
    out["sheet"] = _case(np.c_[gv, np.full(64, 0.53125)], gt, np.c_[sheet, np.full(400, 0.5)], ks=(8, 16), degenerate=True)
    # a collinear cloud (y = z = 1/2) and a zigzag strip of vertices beside it: rank-1 M
    lx = np.sort(rng.uniform(0.0, 1.0, 40))
    lv = np.c_[np.linspace(0.1, 0.9, 12), 0.5625 + 0.03125 * (np.arange(12) % 2), np.full(12, 0.46875)]
    lt = _strip(12)
    out["line"] = _case(lv, lt, np.c_[lx, np.full(40, 0.5), np.full(40, 0.5)], ks=(8, 16), degenerate=True)
    # N = k coincident particles: tau = 0, the mesh only translates
    out["coincident"] = _case(c + 0.1 * icosphere(0)[0], icosphere(0)[1], np.tile(_f32([[0.3, 0.4, 0.5]]), (16, 1)), ks=(16,),
                              tie_free=False, degenerate=True)
    # vertices exactly on particles: d2_0 = 0
    on = _f32(cloud)[100:150].astype(np.float64)
    out["on_particles"] = _case(on, _strip(50), cloud, ks=(8, 16))
    # an integer lattice cloud with vertices on lattice points and cell centres: many exact distance ties
    ix = np.arange(8, dtype=np.float64)
    ints = np.stack(np.meshgrid(ix, ix, ix, indexing="ij"), -1).reshape(-1, 3)
    pick = np.random.default_rng(11).permutation(len(ints))[:20]
    tv = np.concatenate([ints[pick[:10]], ints[pick[10:]] % 7 + 0.5])
    out["ties"] = _case(tv, _strip(20), ints, ks=(8, 16), tie_free=False)
    # poles of valence 100 in one workgroup's stretch of corners, which spans several LDS chunks
    pv, pt = uv_sphere(100, 5)
    out["poles"] = _case(c + 0.3 * pv, pt, cloud, ks=(16,))
    # odd topology: vertex 4 isolated, a triangle with a repeated index, and a fan that cancels exactly (one triangle, both windings)
    ov = c + 0.3 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, 0.3, 0.3], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.float64)
    ot = [(0, 1, 2), (0, 2, 3), (1, 1, 3), (5, 6, 7), (5, 7, 6)]
    out["odd"] = _case(ov, ot, cloud, ks=(16,), zero_normals=(4, 5, 6, 7))
    out["no_triangles"] = _case(c + 0.3 * icosphere(0)[0], np.zeros((0, 3)), cloud, ks=(16,), zero_normals=tuple(range(12)))
    return out


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


AFFINE = _rot((1.0, 2.0, -1.5), 170.0) @ np.array([[1.3, 0.25, 0.0], [0.0, 0.8, -0.15], [0.0, 0.0, 1.1]])
SHIFT = np.array([0.37, -1.25, 2.0])


def motions():
    """name -> (map on fp64 points, (A, b) for the affine ones or None).  The moved particles are rounded to fp32 by the caller."""
    def twist(P):
        ang = 2.5 * (P[:, 2] - 0.5)
        cs, sn = np.cos(ang), np.sin(ang)
        x, y = P[:, 0] - 0.5, P[:, 1] - 0.5
        return np.stack([0.5 + cs * x - sn * y, 0.5 + sn * x + cs * y, P[:, 2] + 0.1 * x * x], 1)
    return {"identity": (lambda P: P.copy(), (np.eye(3), np.zeros(3))),
            "translation": (lambda P: P + SHIFT, (np.eye(3), SHIFT)),
            "affine": (lambda P: P @ AFFINE.T + SHIFT, (AFFINE, SHIFT)),
            "twist": (twist, None)}


def moved(X, name):
    """the fp32 particle state of motion `name` applied to the fp32 rest particles X"""
    return np.ascontiguousarray(motions()[name][0](np.asarray(X, dtype=np.float64)).astype(np.float32))


OBJ_TEXT = """# a quad and a triangle with uv, normals, a material and negative indices
mtllib scene.mtl
o patch
v 0.25 0.25 0.5 1.0 0.5 0.25
v 0.75 0.25 0.5
v 0.75 0.75 0.5

v 0.25 0.75 0.5
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 0 1
vn 0 0 1
g front
usemtl red
s off
f 1/1/1 2/2/1  3/3/2 4/4/2
v 0.5 0.5 0.75
# the apex, addressed from the end
usemtl blue
f -1//2 1//1 2//1
f -5/1 -4/2 -1/3
"""
