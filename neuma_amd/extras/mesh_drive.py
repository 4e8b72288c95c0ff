"""Driven meshes in numpy fp64: the definition, the CPU path of neuma_amd/mesh_drive.py and the yardstick of csrc/nm_meshdrive.hip
(no reference counterpart: the reference only ever shows Gaussians).

A mesh V0 (V, 3), triangles (T, 3) lies in the frame of the rest particles X (N, 3); all are fp32 values, the arithmetic is fp64.
A vertex follows its k nearest rest particles (1 <= k <= 16) by an affine moving-least-squares fit, written as fixed coefficients:

  neighbours   i_0 .. i_{k-1}: the k particles with the smallest (d2, index), d2 ascending (knn_brute; nm_knn on the GPU)
  weights      R2 = 1.21 d2_{k-1};  w_j = (1 - d2_j / R2)^2, all 1 when R2 == 0;  w^_j = w_j / sum w_j
  moments      Xbar = sum w^_j X_j, evaluated as X_0 + sum w^_j (X_j - X_0) so that coincident, collinear and coplanar neighbours
               give moments that vanish exactly where they should;  y_j = X_j - Xbar;  M = sum w^_j y_j y_j^T;  tau = tr M;
               r = V0_v - Xbar
  damped fit   g = (M M + (eps tau)^2 I)^-1 M r, 0 when tau == 0 (eps = damping): smooth, no rank threshold; a direction in which
               the neighbours have no extent contributes nothing and the vertex only translates along it
  coefficients c_j = w^_j (1 + y_j . g);  sum c_j = 1 in exact arithmetic
  frame        v(x) = V0_v + sum_j c_j (x_j - X_j): frame 0 is the input bit for bit; an affine motion x = A X + b gives
               A V0 + b - (A - I) delta, delta's component along eigenvector i of M being (eps tau)^2 / (l_i^2 + (eps tau)^2) r_i

Every sum over j runs j = 0 .. k-1 in that order, and the 3x3 system is solved by L D L^T on M / tau (trace 1), operation for
operation what the kernel does.  Vertex normals are area-weighted (normals); vertex values are the w^-weighted mean of the
neighbours' (vertex_values, the rule of field_paint over a CSR)."""
import re
from typing import Dict, Tuple

import numpy as np

MAX_K = 16
DEFAULT_K = 16
DEFAULT_DAMPING = 1e-5


def _f32_as_f64(a, name: str, cols: int = 3) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{name}: shape (n, {cols}) expected, got {a.shape}")
    a = a.astype(np.float32).astype(np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: non-finite values")
    return a


def check_triangles(triangles, n_verts: int) -> np.ndarray:
    """(T, 3) int32; ValueError on an index outside [0, n_verts).  A repeated index is allowed (the triangle counts for nothing)."""
    t = np.asarray(triangles)
    if t.size == 0:
        return np.zeros((0, 3), dtype=np.int32)
    if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"triangles: integer shape (T, 3) expected, got {t.dtype} {t.shape}")
    if t.min() < 0 or t.max() >= n_verts:
        raise ValueError(f"triangles: index outside [0, {n_verts})")
    return np.ascontiguousarray(t.astype(np.int32))


def check_k(k, n_particles: int, damping) -> Tuple[int, float]:
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k} outside 1..{MAX_K}")
    if n_particles < k:
        raise ValueError(f"{n_particles} particles are fewer than k = {k}")
    damping = float(damping)
    if not (np.isfinite(damping) and damping > 0):
        raise ValueError(f"damping must be finite and > 0, got {damping}")
    return k, damping


def knn_brute(V0, X, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """(idx (V, k) int64, d2 (V, k) fp64): for every vertex the k particles with the smallest (d2, index) in lexicographic order,
    d2 = (dx dx + dy dy) + dz dz in fp64 from the fp32 coordinates - what nm_knn returns."""
    V0, X = _f32_as_f64(V0, "vertices"), _f32_as_f64(X, "particles")
    k, _ = check_k(k, len(X), 1.0)
    idx = np.empty((len(V0), k), dtype=np.int64)
    d2 = np.empty((len(V0), k), dtype=np.float64)
    for i0 in range(0, len(V0), 256):
        d = V0[i0:i0 + 256, None, :] - X[None, :, :]
        q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        o = np.argsort(q, axis=1, kind="stable")[:, :k]                         # stable: ties by ascending index
        idx[i0:i0 + 256] = o
        d2[i0:i0 + 256] = np.take_along_axis(q, o, axis=1)
    return idx, d2


def bind(V0, X, idx, d2, damping: float = DEFAULT_DAMPING):
    """(col (V, k) int32, c (V, k) fp64, w_hat (V, k) fp64, info) from the neighbour lists (idx, d2) of knn_brute / nm_knn.
    info, per vertex, of M^ = M / tau: `eig` (V, 3) its eigenvalues ascending (they sum to 1; zeros where tau == 0), `cond` the
    condition number (l_max^2 + eps^2) / (l_min^2 + eps^2) of M^ M^ + eps^2 I (1 where tau == 0), `tau`, `r`, `g`, `y` (V, k, 3)."""
    V0, X = _f32_as_f64(V0, "vertices"), _f32_as_f64(X, "particles")
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=np.float64)
    nv, k = idx.shape
    k, eps = check_k(k, len(X), damping)
    if d2.shape != idx.shape or len(V0) != nv:
        raise ValueError(f"idx {idx.shape}, d2 {d2.shape} for {len(V0)} vertices")
    if nv and (idx.min() < 0 or idx.max() >= len(X)):
        raise ValueError(f"idx: index outside [0, {len(X)})")
    R2 = 1.21 * d2[:, k - 1]
    pos = R2 > 0
    w = np.ones_like(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 1.0 - d2 / R2[:, None]
    w[pos] = (t * t)[pos]
    W = np.zeros(nv)
    for j in range(k):
        W = W + w[:, j]
    w_hat = w / W[:, None]
    Xn = X[idx]                                                                # (V, k, 3)
    xb = np.zeros((nv, 3))                                                     # summed from the nearest neighbour (see above)
    for j in range(k):
        xb = xb + w_hat[:, j, None] * (Xn[:, j] - Xn[:, 0])
    xb = Xn[:, 0] + xb
    y = Xn - xb[:, None, :]
    M = np.zeros((nv, 3, 3))
    for j in range(k):
        wy = w_hat[:, j, None] * y[:, j]
        M = M + wy[:, :, None] * y[:, j, None, :]
    tau = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    r = V0 - xb
    live = tau > 0
    ts = np.where(live, tau, 1.0)
    H = M / ts[:, None, None]
    H = np.stack([np.stack([H[:, 0, 0], H[:, 0, 1], H[:, 0, 2]], 1), np.stack([H[:, 0, 1], H[:, 1, 1], H[:, 1, 2]], 1),
                  np.stack([H[:, 0, 2], H[:, 1, 2], H[:, 2, 2]], 1)], 1)        # the upper triangle, mirrored: what the kernel holds
    e2 = eps * eps
    A = np.empty((nv, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            A[:, a, b] = (H[:, a, 0] * H[:, 0, b] + H[:, a, 1] * H[:, 1, b]) + H[:, a, 2] * H[:, 2, b]
            if a == b:
                A[:, a, b] = A[:, a, b] + e2
    rhs = np.stack([(H[:, a, 0] * r[:, 0] + H[:, a, 1] * r[:, 1]) + H[:, a, 2] * r[:, 2] for a in range(3)], 1)
    p0 = A[:, 0, 0]
    l10, l20 = A[:, 0, 1] / p0, A[:, 0, 2] / p0
    p1 = A[:, 1, 1] - l10 * A[:, 0, 1]
    t21 = A[:, 1, 2] - l20 * A[:, 0, 1]
    l21 = t21 / p1
    p2 = (A[:, 2, 2] - l20 * A[:, 0, 2]) - l21 * t21
    z0 = rhs[:, 0]
    z1 = rhs[:, 1] - l10 * z0
    z2 = (rhs[:, 2] - l20 * z0) - l21 * z1
    z0, z1, z2 = z0 / p0, z1 / p1, z2 / p2
    x2 = z2
    x1 = z1 - l21 * x2
    x0 = (z0 - l10 * x1) - l20 * x2
    g = np.stack([x0, x1, x2], 1) / ts[:, None]
    g[~live] = 0.0
    dot = (y[:, :, 0] * g[:, None, 0] + y[:, :, 1] * g[:, None, 1]) + y[:, :, 2] * g[:, None, 2]
    c = w_hat * (1.0 + dot)
    eig = np.clip(np.linalg.eigvalsh(H), 0.0, None) if nv else np.zeros((0, 3))
    eig[~live] = 0.0
    cond = np.where(live, (eig[:, 2] ** 2 + e2) / (eig[:, 0] ** 2 + e2), 1.0)
    info = dict(eig=eig, cond=cond, tau=tau, r=r, g=g, y=y, H=H)
    return idx.astype(np.int32), c, w_hat, info


def drive(V0, col, c, X, x) -> np.ndarray:
    """V0 + sum_j c_j (x[col_j] - X[col_j]) in fp64, j ascending: the frame's vertex positions (V, 3)."""
    V0, X, x = _f32_as_f64(V0, "vertices"), _f32_as_f64(X, "rest particles"), _f32_as_f64(x, "particles")
    if x.shape != X.shape:
        raise ValueError(f"{len(x)} particles for a mesh bound to {len(X)}")
    col = np.asarray(col, dtype=np.int64)
    c = np.asarray(c, dtype=np.float64)
    u = x - X
    out = np.zeros_like(V0)
    for j in range(col.shape[1]):
        out = out + c[:, j, None] * u[col[:, j]]
    return V0 + out


def vertex_values(w_hat, col, q) -> np.ndarray:
    """q_v = (sum_j w^_j q[col_j]) / (sum_j w^_j): NaN where a neighbour's value is not finite (field_paint's rule over a CSR)."""
    w_hat = np.asarray(w_hat, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    qn = q[np.asarray(col, dtype=np.int64)]
    num, den = np.zeros(len(w_hat)), np.zeros(len(w_hat))
    for j in range(w_hat.shape[1]):
        num = num + w_hat[:, j] * np.where(np.isfinite(qn[:, j]), qn[:, j], 0.0)
        den = den + w_hat[:, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / den
    out[~np.isfinite(qn).all(1) | (den == 0)] = np.nan
    return out


def corner_adjacency(triangles, n_verts: int) -> Tuple[np.ndarray, np.ndarray]:
    """(vptr (V + 1) int32, vcorner (3 T) int32): the corner ids 3 t + c sorted by (vertex, corner id); vertex v's incident
    corners are vcorner[vptr[v] : vptr[v + 1]], ascending."""
    t = check_triangles(triangles, n_verts)
    flat = t.reshape(-1).astype(np.int64)
    if 3 * len(t) >= 2 ** 31:
        raise ValueError(f"{len(t)} triangles: 3 T does not fit an int32")
    vcorner = np.argsort(flat, kind="stable").astype(np.int32)
    vptr = np.zeros(n_verts + 1, dtype=np.int64)
    vptr[1:] = np.cumsum(np.bincount(flat, minlength=n_verts))
    return vptr.astype(np.int32), vcorner


def normals(P, triangles, vptr=None, vcorner=None) -> np.ndarray:
    """Area-weighted vertex normals (V, 3) fp64: vertex v sums (p_next - p_v) x (p_prev - p_v) over its incident corners in ascending
    corner id (a triangle with a repeated index adds zero), scales the sum by its largest |component| and normalises it; (0, 0, 0)
    for a zero or non-finite sum (an isolated vertex, a fan that cancels)."""
    P = np.asarray(P, dtype=np.float64)
    t = check_triangles(triangles, len(P)).astype(np.int64)
    if vptr is None:
        vptr, vcorner = corner_adjacency(t, len(P))
    cid = np.asarray(vcorner, dtype=np.int64)
    tt, cc = cid // 3, cid % 3
    iv, inx, ipv = t[tt, cc], t[tt, (cc + 1) % 3], t[tt, (cc + 2) % 3]
    s = np.zeros((len(P), 3))
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.cross(P[inx] - P[iv], P[ipv] - P[iv]) if len(cid) else np.zeros((0, 3))
        tri = t[tt]
        cr[(tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])] = 0.0
        np.add.at(s, iv, cr)                                                   # unbuffered: in the order of vcorner
    m = np.abs(s).max(1) if len(P) else np.zeros(0)
    ok = np.isfinite(s).all(1) & (m > 0)
    out = np.zeros_like(s)
    sn = s[ok] / m[ok, None]
    out[ok] = sn / np.sqrt((sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2])[:, None]
    return out


def edge_ratio(P, P0, triangles) -> float:
    """The largest edge length of P over the same edge's length in P0 (edges of zero rest length are left out; 1 with no edge)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if not len(t):
        return 1.0
    a, b = t.reshape(-1), np.roll(t, -1, axis=1).reshape(-1)
    P, P0 = np.asarray(P, dtype=np.float64), np.asarray(P0, dtype=np.float64)
    l0 = np.sqrt(((P0[a] - P0[b]) ** 2).sum(1))
    l1 = np.sqrt(((P[a] - P[b]) ** 2).sum(1))
    keep = l0 > 0
    return float((l1[keep] / l0[keep]).max()) if keep.any() else 1.0


# ------------------------------------------------------------------ Wavefront OBJ, kept as it is

_CORNER = re.compile(r"(-?\d+)/(-?\d*)/-?\d+")


def read_obj(text: str) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices (V, 3) fp64, triangles (T, 3) int64) of an OBJ text: `v` and `f` records, polygons fan-triangulated, negative
    indices relative to the vertices read so far."""
    verts, tris = [], []
    for line in text.splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            verts.append([float(a) for a in tok[1:4]])
        elif tok[0] == "f":
            idx = [int(a.split("/")[0]) for a in tok[1:]]
            idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
            tris += [(idx[0], idx[i], idx[i + 1]) for i in range(1, len(idx) - 1)]
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def rewrite_obj(text: str, positions) -> str:
    """The OBJ `text` with the n-th `v` line carrying positions[n] (fp32, nine digits: exact; what follows x y z on the line, a
    colour say, stays), `vn` lines dropped and face corners without their normal index (a/b/c -> a/b, a//c -> a).  Every other
    byte is kept: comments, `vt`, `usemtl`, `mtllib`, groups, polygon faces, blank lines, line endings."""
    P = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    out, n = [], 0
    for line in text.splitlines(keepends=True):
        tok = line.split()
        head = tok[0] if tok else ""
        if head == "v":
            if n >= len(P):
                raise ValueError(f"the OBJ has more than {len(P)} `v` lines")
            body = line.rstrip("\r\n")
            rest = "".join(" " + a for a in tok[4:])
            out.append("v %.9g %.9g %.9g%s%s" % (P[n, 0], P[n, 1], P[n, 2], rest, line[len(body):]))
            n += 1
        elif head == "vn":
            continue
        elif head == "f":
            out.append(_CORNER.sub(lambda m: m.group(1) + ("/" + m.group(2) if m.group(2) else ""), line))
        else:
            out.append(line)
    if n != len(P):
        raise ValueError(f"the OBJ has {n} `v` lines for {len(P)} positions")
    return "".join(out)


def describe(n_verts: int, n_tris: int, k: int, c, d2) -> Dict:
    """What a driver prints at bind: max sum |c_j| (a bad embedding shows here: hundreds for near-coplanar neighbourhoods) and the
    largest nearest-particle distance over the median one."""
    c = np.asarray(c, dtype=np.float64)
    d = np.sqrt(np.asarray(d2, dtype=np.float64)[:, 0]) if n_verts else np.zeros(0)
    med = float(np.median(d)) if n_verts else 0.0
    return dict(V=int(n_verts), T=int(n_tris), k=int(k), max_abs_c=float(np.abs(c).sum(1).max()) if n_verts else 0.0,
                far=float(d.max() / med) if med > 0 else (0.0 if not n_verts or d.max() == 0 else float("inf")))
