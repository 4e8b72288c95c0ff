// Exact point-in-mesh test on the device: the ray-parity count of extras/mesh_sampling.py points_in_mesh (a ray along +z from
// every point, a hit per triangle whose fp64 barycentrics in xy are all >= 0 and whose interpolated z lies above the point),
// bit for bit.  The triangles are binned into a uniform xy cell grid, so that each point only evaluates the triangles of
// its own cell:
//   k_mi_prep     one thread per triangle: index check, the operands the test reads (d included), the `ok` filter, a
//                 conservative xy box (below), and a partial xy box of the mesh per workgroup
//   k_mi_grid     one workgroup: finish of the partials -> the mesh's xy box and its cells (nm_cells_fit of nm_cells.h, within
//                 a cell budget that depends on the triangle count only, so the host sizes the workspace without reading the data)
//   k_mi_count    cell range of every triangle's box, per-cell counters (integer atomics).  A triangle whose box covers more
//                 than kMaxCells cells, whose cells no longer fit the pair capacity, or that has no finite box, goes to the
//                 list that every point walks instead
//   (rocPRIM exclusive scan of the counters)
//   k_mi_scatter  the triangle ids by cell
//   k_mi_query    one thread per point: the triangles of its cell, then the walk-all list; inside = odd hit count
// Every candidate a point meets is evaluated with the exact formula, so binning only prunes.  The count is an integer, so the
// result does not depend on the order of triangles inside a cell (which the atomics leave open).  No float atomics, no host
// synchronisation: two calls give identical bytes.
//
// The formula is evaluated as numpy evaluates it, one rounded operation at a time: no contraction into fma (numpy does not
// fuse; the Makefile also passes -ffp-contract=off for this file), and fp64 `/` is the correctly rounded division.
#include "nm_cells.h"
#include "nm_reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMiThreads = 256;
constexpr int kMiMaxBlocks = 1024;   // k_mi_prep workgroups (each writes one partial box)
constexpr int kTrisPerCell = 4;      // cell budget = ceil(T / 4)
constexpr int kMaxCells = 64;        // a triangle covering more cells goes to the walk-all list
constexpr int kPairsPerTri = 8;      // (triangle, cell) pair capacity = 8 T + 64
constexpr int kMaxTris = 1 << 27;

// the numpy formula's per-triangle operands (a, b, c = the triangle's vertices):
//   l0 = (e0 * (px - c0) + e1 * (py - c1)) / d      e0 = b1 - c1, e1 = c0 - b0
//   l1 = (f0 * (px - c0) + f1 * (py - c1)) / d      f0 = c1 - a1, f1 = a0 - c0
//   d  = e0 * f1 + e1 * (a1 - c1)
struct MiTri {
  double c0, c1, e0, e1, f0, f1, d, a2, b2, c2;
};

struct MiBoxPart {
  double lo[2], hi[2];
};

using MiGrid = NmCells<2>;      // boxes and points alike go through nm_cell

// per-triangle state between the passes (0 = boxed, not yet placed)
enum : int { kTriDropped = -1, kTriAll = -2, kTriBinned = 1 };

static inline int mi_cell_budget(int t) { return t <= kTrisPerCell ? 1 : (int)(((int64_t)t + kTrisPerCell - 1) / kTrisPerCell); }
static inline int mi_prep_blocks(int t) {
  const int g = nm_div_up(t, kMiThreads);
  return g < 1 ? 1 : (g > kMiMaxBlocks ? kMiMaxBlocks : g);
}
static inline int64_t mi_pair_cap(int t) { return (int64_t)kPairsPerTri * t + 64; }

struct MiWs {
  int gprep, cmax;
  int64_t cap;
  MiTri* rec;                  // T
  double4* box;                // T: {lo x, lo y, hi x, hi y}
  int* state;                  // T
  MiBoxPart* part;             // gprep
  MiGrid* grid;
  unsigned long long* used;    // pairs reserved so far
  int* nall;                   // length of the walk-all list
  int* cnt;                    // cmax + 1 counters
  int* start;                  // their exclusive scan
  int* pairs;                  // cap triangle ids, by cell
  int* all;                    // T triangle ids
  NmIntScan scan;
  size_t total;
};

static MiWs carve(void* base, int t) {
  MiWs w;
  w.gprep = mi_prep_blocks(t); w.cmax = mi_cell_budget(t); w.cap = mi_pair_cap(t);
  const size_t nt = t > 0 ? (size_t)t : 1, nc = (size_t)w.cmax + 1;
  NmCarver c(base);
  w.rec = c.take<MiTri>(nt);
  w.box = c.take<double4>(nt);
  w.state = c.take<int>(nt);
  w.part = c.take<MiBoxPart>(w.gprep);
  w.grid = c.take<MiGrid>(1);
  w.used = c.take<unsigned long long>(1);                    // used and nall share one 256-byte slot, cleared together
  w.nall = (int*)(w.used + 1);
  w.cnt = c.take<int>(nc);
  w.start = c.take<int>(nc);
  w.pairs = c.take<int>((size_t)w.cap);
  w.all = c.take<int>(nt);
  w.scan.carve(c, nc);
  w.total = c.total();
  return w;
}

__device__ __forceinline__ bool mi_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// The conservative box.  Say the test reports a hit at p: the computed l0, l1 >= 0 and l2 = (1 - l0) - l1 >= 0.  Rounding is
// monotone, so fl(fl(1 - l0) - l1) >= 0 gives l1 <= fl(1 - l0), hence l0 + l1 <= 1 + u (u = 2^-53).  With dx = fl(px - c0),
// dy = fl(py - c1) and M = [e0 e1; f0 f1] (det M = e0 f1 - e1 f0 is the exact value of d's expression), the numerators are
// M (dx, dy) + err with |err_i| <= g2 |row_i| . |(dx, dy)| (g2 = 2u / (1 - 2u)), and they equal l_i d / (1 + delta), |delta| <= u.
// So (dx, dy) = (d / det) / (1 + delta) adj(M) l - adj(M) err / det, and adj(M) l = l0 (a - c) + l1 (b - c) (edges as rounded)
// is a point of the triangle scaled by 1 + u about c.  With E = max(|e0|, |e1|, |f0|, |f1|) and X = max(|dx|, |dy|):
// |d / det - 1| <= 2 g2 E^2 / |det| and |adj(M) err| <= 4 g2 E^2 X.  With k = 4 g2 E^2 / |det| <= 1/4 this puts the hit point
// within 2.2 k E + 6 u E (max norm) of the triangle, the rounding of dx, dy and of the edges included; and lo - m, hi + m
// round by at most u (|x| + m).  So m = (4 k + 16 u) E + 4 u C (C = the largest |vertex coordinate| in xy) is a safe margin,
// here with k = 10 u E^2 / |det|low and |det|low = |d| - 4 u (|e0 f1| + |e1 (a1 - c1)|), a lower bound on |det|.
// A triangle with k > 1/4 (a sliver, nearly collinear in xy) or a non-finite box gets no box: every point tests it.
__global__ void __launch_bounds__(kMiThreads) k_mi_prep(int T, int V, const double* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        MiTri* __restrict__ rec, double4* __restrict__ box, int* __restrict__ state,
                                                        MiBoxPart* __restrict__ part) {
  constexpr int NW = kMiThreads / 64;
  __shared__ double red[NW * 4];
  double bb[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};      // lo x, lo y, hi x, hi y
  const int stride = gridDim.x * kMiThreads;
  for (int t = blockIdx.x * kMiThreads + threadIdx.x; t < T; t += stride) {
    const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {    // never read out of range: dropped
      state[t] = kTriDropped;
      continue;
    }
    const double a0 = verts[3 * (size_t)ia], a1 = verts[3 * (size_t)ia + 1], a2 = verts[3 * (size_t)ia + 2];
    const double b0 = verts[3 * (size_t)ib], b1 = verts[3 * (size_t)ib + 1], b2 = verts[3 * (size_t)ib + 2];
    const double c0 = verts[3 * (size_t)ic], c1 = verts[3 * (size_t)ic + 1], c2 = verts[3 * (size_t)ic + 2];
    MiTri r;
    r.c0 = c0; r.c1 = c1;
    r.e0 = b1 - c1; r.e1 = c0 - b0;
    r.f0 = c1 - a1; r.f1 = a0 - c0;
    const double g1 = a1 - c1;
    const double p0 = r.e0 * r.f1, p1 = r.e1 * g1;
    r.d = p0 + p1;
    r.a2 = a2; r.b2 = b2; r.c2 = c2;
    rec[t] = r;
    if (!(fabs(r.d) > 1e-300)) {          // numpy's `ok` filter (a NaN fails it too)
      state[t] = kTriDropped;
      continue;
    }
    const double u = 0x1p-53;
    const double E = fmax(fmax(fabs(r.e0), fabs(r.e1)), fmax(fabs(r.f0), fabs(r.f1)));
    const double C = fmax(fmax(fmax(fabs(a0), fabs(a1)), fmax(fabs(b0), fabs(b1))), fmax(fabs(c0), fabs(c1)));
    const double detlow = fabs(r.d) - 4.0 * u * (fabs(p0) + fabs(p1));
    const double k = detlow > 0.0 ? 10.0 * u * (E * E) / detlow : INFINITY;
    const double m = (4.0 * k + 16.0 * u) * E + 4.0 * u * C;
    const double4 bx = make_double4(fmin(fmin(a0, b0), c0) - m, fmin(fmin(a1, b1), c1) - m, fmax(fmax(a0, b0), c0) + m,
                                    fmax(fmax(a1, b1), c1) + m);
    const bool boxed = k <= 0.25 && mi_finite(bx.x) && mi_finite(bx.y) && mi_finite(bx.z) && mi_finite(bx.w);
    box[t] = bx;
    state[t] = boxed ? 0 : kTriAll;
    if (boxed) {               // the grid spans the boxed triangles' vertices (points and boxes beyond it clamp to its edge)
      bb[0] = fmin(bb[0], fmin(fmin(a0, b0), c0)); bb[1] = fmin(bb[1], fmin(fmin(a1, b1), c1));
      bb[2] = fmax(bb[2], fmax(fmax(a0, b0), c0)); bb[3] = fmax(bb[3], fmax(fmax(a1, b1), c1));
    }
  }
  const auto tot = nm_block_reduce<NW, NmMinMax<2>>(bb, red);
  if (threadIdx.x == 0) {
    MiBoxPart p;
#pragma unroll
    for (int j = 0; j < 2; ++j) { p.lo[j] = tot[j]; p.hi[j] = tot[2 + j]; }
    part[blockIdx.x] = p;
  }
}

// one workgroup: the mesh's xy box, then square cells within the budget (an axis shorter than the cell edge gets one cell)
__global__ void __launch_bounds__(kMiThreads) k_mi_grid(int gprep, int cmax, const MiBoxPart* __restrict__ part, MiGrid* __restrict__ grid) {
  constexpr int NW = kMiThreads / 64;
  __shared__ double red[NW * 4];
  double bb[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};      // lo x, lo y, hi x, hi y
  for (int g = threadIdx.x; g < gprep; g += kMiThreads) {
    const MiBoxPart p = part[g];
    bb[0] = fmin(bb[0], p.lo[0]); bb[1] = fmin(bb[1], p.lo[1]); bb[2] = fmax(bb[2], p.hi[0]); bb[3] = fmax(bb[3], p.hi[1]);
  }
  const auto tot = nm_block_reduce<NW, NmMinMax<2>>(bb, red);
  if (threadIdx.x != 0) return;
  double lo[2] = {tot[0], tot[1]}, hi[2] = {tot[2], tot[3]}, e[2];
  MiGrid G;
  nm_cells_fit(lo, hi, cmax, G, e);                            // (no boxed triangle, or a span beyond the fp64 range: one cell)
  *grid = G;
}

__global__ void __launch_bounds__(kMiThreads) k_mi_count(int T, long long cap, const double4* __restrict__ box,
                                                         const MiGrid* __restrict__ grid, int* __restrict__ state, int* __restrict__ cnt,
                                                         unsigned long long* __restrict__ used, int* __restrict__ nall,
                                                         int* __restrict__ all) {
  const int t = blockIdx.x * kMiThreads + threadIdx.x;
  if (t >= T) return;
  const int st = state[t];
  if (st == kTriDropped) return;
  bool binned = false;
  if (st == 0) {
    const MiGrid G = *grid;
    const double4 b = box[t];
    const int x0 = nm_cell(b.x, G.o[0], G.inv_h[0], G.n[0]), x1 = nm_cell(b.z, G.o[0], G.inv_h[0], G.n[0]);
    const int y0 = nm_cell(b.y, G.o[1], G.inv_h[1], G.n[1]), y1 = nm_cell(b.w, G.o[1], G.inv_h[1], G.n[1]);
    const int nc = (x1 - x0 + 1) * (y1 - y0 + 1);
    if (nc <= kMaxCells && (long long)(atomicAdd(used, (unsigned long long)nc) + nc) <= cap) {
      binned = true;
      for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) atomicAdd(&cnt[x * G.n[1] + y], 1);
    }
  }
  if (binned) {
    state[t] = kTriBinned;
  } else {
    state[t] = kTriAll;
    all[atomicAdd(nall, 1)] = t;
  }
}

__global__ void __launch_bounds__(kMiThreads) k_mi_scatter(int T, const double4* __restrict__ box, const MiGrid* __restrict__ grid,
                                                           const int* __restrict__ state, const int* __restrict__ start,
                                                           int* __restrict__ cnt, int* __restrict__ pairs) {
  const int t = blockIdx.x * kMiThreads + threadIdx.x;
  if (t >= T || state[t] != kTriBinned) return;
  const MiGrid G = *grid;
  const double4 b = box[t];
  const int x0 = nm_cell(b.x, G.o[0], G.inv_h[0], G.n[0]), x1 = nm_cell(b.z, G.o[0], G.inv_h[0], G.n[0]);
  const int y0 = nm_cell(b.y, G.o[1], G.inv_h[1], G.n[1]), y1 = nm_cell(b.w, G.o[1], G.inv_h[1], G.n[1]);
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const int c = x * G.n[1] + y;
      pairs[start[c] + atomicSub(&cnt[c], 1) - 1] = t;       // (the counters count back down to 0)
    }
}

// numpy's test of one (point, triangle) pair, operation for operation
__device__ __forceinline__ int mi_hit(const MiTri& r, double px, double py, double pz) {
  const double dx = px - r.c0, dy = py - r.c1;
  const double l0 = (r.e0 * dx + r.e1 * dy) / r.d;
  const double l1 = (r.f0 * dx + r.f1 * dy) / r.d;
  const double l2 = (1.0 - l0) - l1;
  if (!(l0 >= 0.0 && l1 >= 0.0 && l2 >= 0.0)) return 0;
  const double z = (l0 * r.a2 + l1 * r.b2) + l2 * r.c2;
  return z > pz ? 1 : 0;
}

__global__ void __launch_bounds__(kMiThreads) k_mi_query(int P, const double* __restrict__ pts, const MiTri* __restrict__ rec,
                                                         const MiGrid* __restrict__ grid, const int* __restrict__ start,
                                                         const int* __restrict__ pairs, const int* __restrict__ nall,
                                                         const int* __restrict__ all, uint8_t* __restrict__ inside) {
  const int i = blockIdx.x * kMiThreads + threadIdx.x;
  if (i >= P) return;
  const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
  const MiGrid G = *grid;
  const int c = nm_cell(px, G.o[0], G.inv_h[0], G.n[0]) * G.n[1] + nm_cell(py, G.o[1], G.inv_h[1], G.n[1]);
  int hits = 0;
  const int s = start[c], e = start[c + 1];
  for (int k = s; k < e; ++k) hits += mi_hit(rec[pairs[k]], px, py, pz);
  const int na = *nall;
  for (int k = 0; k < na; ++k) hits += mi_hit(rec[all[k]], px, py, pz);
  inside[i] = (uint8_t)(hits & 1);
}

static bool mi_sizes_ok(int32_t n_tris, int32_t n_points) { return n_tris >= 0 && n_tris <= kMaxTris && n_points >= 0; }

}  // namespace

extern "C" size_t nm_mesh_inside_workspace(int32_t n_tris, int32_t n_points) {
  if (!mi_sizes_ok(n_tris, n_points)) return 0;
  return carve(nullptr, n_tris).total;
}

extern "C" int nm_points_in_mesh(int32_t n_verts, int32_t n_tris, int32_t n_points, const double* verts, const int32_t* tris,
                                 const double* points, uint8_t* inside_out, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(n_verts >= 0, "n_verts must be >= 0");
  NM_REQUIRE(mi_sizes_ok(n_tris, n_points), "n_tris must be in [0, 2^27] and n_points >= 0");
  NM_REQUIRE(n_points == 0 || (points && inside_out), "null pointer");
  NM_REQUIRE(n_points == 0 || n_tris == 0 || (tris && (verts || n_verts == 0)), "null pointer");
  NM_REQUIRE(ws && ws_bytes >= nm_mesh_inside_workspace(n_tris, n_points), "workspace too small (nm_mesh_inside_workspace)");
  if (n_points == 0) return NM_OK;
  const hipStream_t s = (hipStream_t)stream;
  if (n_tris == 0) {
    NM_HIP_CHECK(hipMemsetAsync(inside_out, 0, (size_t)n_points, s));
    return NM_OK;
  }
  const MiWs w = carve(ws, n_tris);
  NM_LAUNCH(k_mi_prep, dim3(w.gprep), dim3(kMiThreads), 0, s, n_tris, n_verts, verts, tris, w.rec, w.box, w.state, w.part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_mi_grid, dim3(1), dim3(kMiThreads), 0, s, w.gprep, w.cmax, (const MiBoxPart*)w.part, w.grid);
  NM_LAUNCH_CHECK();
  const size_t nc = (size_t)w.cmax + 1;
  NM_HIP_CHECK(hipMemsetAsync(w.used, 0, 256, s));
  NM_HIP_CHECK(hipMemsetAsync(w.cnt, 0, nc * sizeof(int), s));
  const dim3 tg(nm_div_up(n_tris, kMiThreads));
  NM_LAUNCH(k_mi_count, tg, dim3(kMiThreads), 0, s, n_tris, (long long)w.cap, (const double4*)w.box, (const MiGrid*)w.grid, w.state,
            w.cnt, w.used, w.nall, w.all);
  NM_LAUNCH_CHECK();
  if (int rc = w.scan.run(w.cnt, w.start, nc, s)) return rc;
  NM_LAUNCH(k_mi_scatter, tg, dim3(kMiThreads), 0, s, n_tris, (const double4*)w.box, (const MiGrid*)w.grid, (const int*)w.state,
            (const int*)w.start, w.cnt, w.pairs);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_mi_query, dim3(nm_div_up(n_points, kMiThreads)), dim3(kMiThreads), 0, s, n_points, points, (const MiTri*)w.rec,
            (const MiGrid*)w.grid, (const int*)w.start, (const int*)w.pairs, (const int*)w.nall, (const int*)w.all, inside_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
