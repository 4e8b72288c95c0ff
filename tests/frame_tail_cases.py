"""Inputs and fp64 references for the frame-tail kernels of csrc/nm_bind.hip (nm_spmm_csr, nm_spmm_csr_sum3, nm_bind_frame,
nm_cov_deform, nm_pixel_loss).  No GPU, no torch: numpy only.

Two kinds of data for every case.

EXACT data lies on dyadic grids - weights k/16 in [1/16, 1], particle / Gaussian values k/16 in [-4, 4], F entries k/4 in
[-4, 4], pixels k/256 (L1) or k/16 (L2) in [0, 1] - so that every product and every partial sum of the operation is a multiple of
one granularity g and smaller than 2^24 g: exactly representable in fp32 whatever the summation order, with or without fma
contraction.  The fp64 reference rounded to fp32 is then the ONLY correct answer and the GPU result is compared bit for bit.
Each builder reports that condition as a `margin` = (largest possible partial sum) / g, which must be < 2^24 (EXACT_LIMIT).

RANDOM data is fp32 normal / uniform, rounded once; the reference is fp64 on the rounded values and the bound is derived:
for a row of L entries |err| <= (L + c) 2^-24 sum_q |w_q| |x_q| (`dot_bound`), c = the elementwise roundings around the dot
product (each GPU test states its c).

The CSR structures are built from CHOSEN row lengths (raw rowptr / col / val), never drawn."""
import math

import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff
EXACT_LIMIT = 2.0 ** 24
NCOLS = 131                     # columns of every structure (>= the longest row, odd)

# rows of the lane-sharing kernels (16 lanes stride a row's entries): below / at / above one and two trips of 16, and long
LANE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 100)
LANE_ROWS = (1, 15, 16, 17, 257)            # one 256-thread workgroup is exactly 16 rows
# rows of k_bind_frame (four entries per trip, masked tail): every residue, the shipped maximum of 10, and long rows
BIND_LENGTHS = tuple(range(11)) + (16, 33)
BIND_K = (1, 255, 256, 257)
SPMM_D = (1, 2, 3, 4, 5, 9, 15, 16, 17, 33)  # D <= 4 lane sharing; 5..16 a lane per column; > 16 the second column trip


class Csr(object):
    """Raw CSR triple (int32, int32, float32) of a rows x ncols matrix; entries of a row ascend in column (a repeated column
    sits next to its twin)."""

    def __init__(self, name, rowptr, col, val, ncols):
        self.name, self.ncols = name, int(ncols)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float32)
        self.rows = int(self.rowptr.shape[0] - 1)
        assert self.rowptr[0] == 0 and self.rowptr[-1] == self.col.shape[0] == self.val.shape[0]
        assert self.col.size == 0 or (0 <= int(self.col.min()) and int(self.col.max()) < self.ncols)

    @property
    def lengths(self):
        return np.diff(self.rowptr.astype(np.int64))

    @property
    def row_of(self):
        return np.repeat(np.arange(self.rows), self.lengths)

    def with_val(self, val):
        return Csr(self.name, self.rowptr, self.col, val, self.ncols)

    def abs(self):
        return self.with_val(np.abs(self.val))

    def dense(self):
        d = np.zeros((self.rows, self.ncols), dtype=np.float64)
        np.add.at(d, (self.row_of, self.col.astype(np.int64)), self.val.astype(np.float64))
        return d

    def row_weight(self):
        """sum_q |w_q| of every row (fp64)"""
        s = np.zeros(self.rows, dtype=np.float64)
        np.add.at(s, self.row_of, np.abs(self.val.astype(np.float64)))
        return s

    def repeated_rows(self):
        """rows that hold one column twice"""
        same = (self.col[1:] == self.col[:-1]) & (self.row_of[1:] == self.row_of[:-1])
        return np.unique(self.row_of[1:][same])


# ---------------------------------------------------------------- data on dyadic grids / random data
def exact_weights(rng, n):
    return (rng.integers(1, 17, size=n) / 16.0).astype(np.float32)          # k/16 in [1/16, 1]


def exact_values(rng, shape):
    return (rng.integers(-64, 65, size=shape) / 16.0).astype(np.float32)    # k/16 in [-4, 4]


def exact_F(rng, shape):
    return (rng.integers(-16, 17, size=shape) / 4.0).astype(np.float32)     # k/4 in [-4, 4]


def random_weights(rng, n):
    return rng.uniform(0.0, 1.0, size=n).astype(np.float32)


def random_values(rng, shape):
    return rng.standard_normal(size=shape).astype(np.float32)


# ---------------------------------------------------------------- structures
def _lengths(kind, rows):
    if kind == "lane":
        if rows == 1:
            return [100]
        mid = [1, 15, 16, 17, 31, 32, 33, 48, 100, 0, 0]
    else:
        if rows == 1:
            return [10]
        mid = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 33, 0, 0]
    return [0] + [mid[i % len(mid)] for i in range(rows - 2)] + [0]         # first and last row empty, two empties in a row


def structure(name, lengths, seed=0, exact=True, samecol=None, ncols=NCOLS):
    """CSR with the given row lengths.  The first row of >= 2 entries holds column 0 and column ncols-1; the second such row
    repeats a column; `samecol`: every entry points at that one column."""
    rng = np.random.default_rng(seed)
    rowptr, cols, long_rows = [0], [], 0
    for L in lengths:
        assert L <= ncols - 2
        if samecol is not None:
            c = np.full(L, samecol, dtype=np.int64)
        else:
            c = np.sort(rng.choice(np.arange(1, ncols - 1), size=L, replace=False))
            if L >= 2:
                long_rows += 1
                if long_rows == 1:
                    c[0], c[-1] = 0, ncols - 1
                elif long_rows == 2:
                    c[1] = c[0]
        cols.append(c)
        rowptr.append(rowptr[-1] + L)
    n = rowptr[-1]
    val = exact_weights(rng, n) if exact else random_weights(rng, n)
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    return Csr(name, np.asarray(rowptr), col, val, ncols)


def lane_structures(exact=True):
    """structures for nm_spmm_csr (D <= 4 shares a row's entries among 16 lanes) and nm_spmm_csr_sum3"""
    out = [structure(f"lane_r{r}", _lengths("lane", r), seed=100 + r, exact=exact) for r in LANE_ROWS]
    out.append(structure("lane_samecol_r17", _lengths("lane", 17), seed=99, exact=exact, samecol=5))
    return out


def bind_structures(exact=True):
    """structures for nm_bind_frame (one thread per row, four entries per trip)"""
    out = [structure(f"bind_k{k}", _lengths("bind", k), seed=200 + k, exact=exact) for k in BIND_K]
    out.append(structure("bind_samecol_k17", _lengths("bind", 17), seed=98, exact=exact, samecol=NCOLS - 1))
    return out


def by_name(structs):
    return {s.name: s for s in structs}


# ---------------------------------------------------------------- references (fp64) and bounds
def spmm_ref(csr, X):
    """A X in fp64 (X: ncols x D)"""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((csr.rows,) + X.shape[1:], dtype=np.float64)
    np.add.at(out, csr.row_of, csr.val.astype(np.float64).reshape((-1,) + (1,) * (X.ndim - 1)) * X[csr.col.astype(np.int64)])
    return out


def spmm_t_ref(csr, G):
    """A^T G in fp64 (G: rows x D)"""
    G = np.asarray(G, dtype=np.float64)
    out = np.zeros((csr.ncols,) + G.shape[1:], dtype=np.float64)
    np.add.at(out, csr.col.astype(np.int64), csr.val.astype(np.float64)[:, None] * G[csr.row_of])
    return out


def transpose(csr):
    """A^T as a Csr (rows ascending in column)"""
    r, c = csr.row_of, csr.col.astype(np.int64)
    order = np.lexsort((r, c))
    rowptr = np.zeros(csr.ncols + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(c, minlength=csr.ncols))
    return Csr(csr.name + "_T", rowptr, r[order], csr.val[order], csr.rows)


def dot_bound(csr, absX, c, extra=0.0):
    """(L + c) 2^-24 (sum_q |w_q| |x_q| + extra) per output element: L roundings of a row's products and partial sums in any
    order plus c elementwise roundings around them (first order; the slack of one unit inside every c covers the higher orders
    for L (L + c) 2^-24 << 1)"""
    L = csr.lengths.astype(np.float64).reshape((-1,) + (1,) * (np.ndim(absX) - 1))
    return (L + c) * U * (spmm_ref(csr.abs(), np.abs(absX)) + extra)


def is_fp32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a, a.astype(np.float32).astype(np.float64)))


def spmm_margin(csr, xmax=4.0, gran=1.0 / 256.0):
    """exactness condition of A X on exact data: weights k/16 times values k/16 are multiples of 1/256, a row's partial sums stay
    below sum_q w_q xmax"""
    return float(csr.row_weight().max(initial=0.0)) * xmax / gran


def bind_frame_margins(csr):
    """(means, F_k): p_cur - p_prev is a multiple of 1/16 in [-8, 8] (exact), its weighted sum a multiple of 1/256, k_prev (<= 4)
    is added last; w F is a multiple of 1/64 below sum_q w_q 4"""
    w = float(csr.row_weight().max(initial=0.0))
    return (w * 8.0 + 4.0) * 256.0, w * 4.0 * 64.0


def sum3_margin(csr, n_in):
    """scale (a power of two) drops out: the n_in inputs add to a multiple of 1/16 in [-4 n, 4 n], the products are multiples
    of 1/256"""
    return float(csr.row_weight().max(initial=0.0)) * 4.0 * n_in * 256.0


def sym6_to_33(c6):
    c6 = np.asarray(c6, dtype=np.float64)
    S = np.empty(c6.shape[:-1] + (3, 3), dtype=np.float64)
    S[..., 0, 0], S[..., 0, 1], S[..., 0, 2] = c6[..., 0], c6[..., 1], c6[..., 2]
    S[..., 1, 0], S[..., 1, 1], S[..., 1, 2] = c6[..., 1], c6[..., 3], c6[..., 4]
    S[..., 2, 0], S[..., 2, 1], S[..., 2, 2] = c6[..., 2], c6[..., 4], c6[..., 5]
    return S


def m33_to_sym6(M):
    return np.stack([M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]], axis=-1)


def cov_push_ref(cov6, F):
    """(F S F^T as six numbers, its elementwise bound 8 2^-24 |F| |S| |F|^T): every element of the fp32 push passes two 3-term
    dot products, 3 roundings each (6); 8 leaves the higher orders room"""
    S, F = sym6_to_33(cov6), np.asarray(F, dtype=np.float64).reshape(-1, 3, 3)
    ref = F @ S @ np.swapaxes(F, -1, -2)
    bound = 8.0 * U * (np.abs(F) @ np.abs(S) @ np.swapaxes(np.abs(F), -1, -2))
    return m33_to_sym6(ref), m33_to_sym6(bound)


# ---------------------------------------------------------------- pixel loss
# (h, w): what the shape reaches in nm_pixel_loss / k_pixel_loss.  3 h w < 65536 for all of them.
PIXEL_SHAPES = {
    (37, 53): dict(vec4=False, grid=111),                   # scalar branch (the existing test's shape), 3h < 128
    (16, 64): dict(vec4=True, grid=48),                     # float4 branch
    (5, 7): dict(vec4=False, grid=15),                      # 3h < 128, rows shorter than a wave
    (43, 260): dict(vec4=True, grid=128, row_trips=2),      # float4; grid of 128 with a second trip over the 129 rows
    (12, 1028): dict(vec4=True, grid=36, col_trips=2),      # float4 inner loop's second trip (w/4 = 257 > 256)
    (12, 1030): dict(vec4=False, grid=36, col_trips=5),     # scalar fallback at w % 4 != 0, long rows
    (1030, 4): dict(vec4=True, grid=512, row_trips=7),      # 512-workgroup cap, float4 branch
    (1030, 5): dict(vec4=False, grid=512, row_trips=7),     # 512-workgroup cap, scalar branch
}


def launch_rule(h, w, aligned=True):
    """nm_pixel_loss's launch, restated: about six image rows per workgroup, 128..512 workgroups (3h of them when there are
    fewer rows than 128); float4 accesses when w % 4 == 0 and all three pointers are 16-byte aligned.  A workgroup walks rows
    blockIdx, blockIdx + grid, ...; a thread walks a row's (vector) columns threadIdx, threadIdx + 256, ..."""
    grid = (3 * h + 5) // 6
    grid = (min(3 * h, 128) if grid < 128 else min(grid, 512))
    vec4 = (w % 4 == 0) and aligned
    row_trips = -(-3 * h // grid)
    col_trips = -(-(w // 4) // 256) if vec4 else -(-w // 256)
    return dict(grid=grid, vec4=vec4, row_trips=row_trips, col_trips=col_trips,
                terms_per_thread=row_trips * col_trips * (4 if vec4 else 1))


def pow2_weight(h, w):
    """(weight, scale): the weight in (1/2, 1] for which weight / (3 h w) is the power of two `scale`"""
    n = 3 * h * w
    p = math.ceil(math.log2(n))
    return n / 2.0 ** p, 2.0 ** -p


def fp32_scale(weight, h, w):
    """the kernel's scale, in its fp32 operations: weight / (3 * h * w)"""
    return np.float32(weight) / (np.float32(3.0) * np.float32(h) * np.float32(w))


def pixel_images(h, w, kind, exact, seed=0):
    """(img, gt) fp32 (3, h, w).  Exact: pixels k/256 (L1) or k/16 (L2) in [0, 1], some of them equal in both images."""
    rng = np.random.default_rng(seed + 7919 * kind + 31 * h + w)
    if not exact:
        return rng.uniform(0, 1, (3, h, w)).astype(np.float32), rng.uniform(0, 1, (3, h, w)).astype(np.float32)
    q = 256 if kind == 0 else 16
    a = rng.integers(0, q + 1, (3, h, w)); b = rng.integers(0, q + 1, (3, h, w))
    same = rng.uniform(size=(3, h, w)) < 0.05
    b[same] = a[same]
    return (a / float(q)).astype(np.float32), (b / float(q)).astype(np.float32)


def pixel_margin(h, w):
    """|d| (L1) and d^2 (L2) are multiples of 1/256 and at most 1: 3 h w terms stay below 2^24 / 256"""
    return 3.0 * h * w * 256.0


def _rows(h, row0, row1):
    return (0, h) if row1 <= row0 else (max(row0, 0), min(row1, h))


def pixel_term_sum(kind, img, gt, row0=0, row1=0):
    """sum of |a - g| or (a - g)^2 over the rows of the stripe, fp64"""
    y0, y1 = _rows(img.shape[1], row0, row1)
    d = img[:, y0:y1].astype(np.float64) - gt[:, y0:y1].astype(np.float64)
    return float(np.abs(d).sum() if kind == 0 else (d * d).sum())


def pixel_loss_ref(kind, weight, img, gt, row0=0, row1=0):
    """weight * mean over the FULL image of the stripe's terms, fp64 (weight as the fp32 number the ABI carries)"""
    return float(np.float32(weight)) * pixel_term_sum(kind, img, gt, row0, row1) / (3.0 * img.shape[1] * img.shape[2])


def pixel_grad_fp32(kind, scale, img, gt, row0=0, row1=0):
    """the gradient as the kernel states it, in numpy fp32: d = fl(a - g); L1: +-scale or 0; L2: fl(fl(2 d) scale) (2 d is
    exact); zero outside the stripe"""
    scale = np.float32(scale)
    d = img.astype(np.float32) - gt.astype(np.float32)
    if kind == 0:
        g = np.where(d > 0, scale, np.where(d < 0, -scale, np.float32(0.0))).astype(np.float32)
    else:
        g = ((np.float32(2.0) * d) * scale).astype(np.float32)
    y0, y1 = _rows(img.shape[1], row0, row1)
    out = np.zeros_like(g)
    out[:, y0:y1] = g[:, y0:y1]
    return out
