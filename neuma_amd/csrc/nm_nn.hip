// Exact 1- and k-nearest-neighbour search between point clouds, batched over B pairs, and the Chamfer distance of
// modules/tune/metrics.py (chamfer_distance_kdtree: one scipy cKDTree per batch item on the host) on the device.
//
// Each cloud is binned once, per batch item, into a uniform grid over its own bounding box:
//   k_nn_box      partial min / max of the finite coordinates and a count of non-finite ones, one per workgroup
//   k_nn_grid     one thread per item: finish of the partials -> the box, its cells (nm_cells_fit of nm_cells.h, within a cell
//                 budget that depends on the cloud's size only, so the host sizes the workspace without knowing the data),
//                 cell edge per axis
//   k_nn_count    cell key of every point, and its rank inside its cell (integer atomics on the cell counters)
//   (rocPRIM exclusive scan of the counters: every cell's first position in the sorted array)
//   k_nn_scatter  the cloud sorted by cell as float4 {x, y, z, index}
// The search (k_nn_search) takes the queries in the sorted order of their own cloud, so that the lanes of a wave start in
// neighbouring cells and walk similar shells.  Each query visits growing shells of target cells around its own (clamped)
// cell and stops once its best squared distance is at most a lower bound on the squared distance to every unvisited cell:
// the distance to the slab beyond each face of the visited block, inside the targets' box (valid for queries outside it).
// Distances are fp64 from the fp32 coordinates, the winner is the lexicographic minimum of (distance^2, target index), so the
// result does not depend on the order of points inside a cell (nor on the atomics' ranks).  The per-item means are fp64 sums in
// the fixed order of nm_reduce.h over the queries in their ORIGINAL order (k_nn_mean_part, k_nn_mean_finish).
// The k-NN search (k_nn_search_k, 1 <= k <= 16: nm_knn, and nm_knn_mean_dist2 = simple_knn's distCUDA2 at k = 3) is the same
// walk with a k-best list per thread in registers; it stops on the k-th best instead of the best.
#include "nm_cells.h"
#include "nm_reduce.h"

namespace {

constexpr int kNnThreads = 256;
constexpr int kBoxMaxBlocks = 64;      // bbox partials per item
constexpr int kMeanMaxBlocks = 64;     // mean partials per item
constexpr int kPointsPerCell = 2;      // cell budget = ceil(P / 2)

struct NnBoxPart {
  float lo[3], hi[3];
  int bad;       // non-finite coordinates seen
  int pad;
};

// One per (cloud, item), written by k_nn_grid.  o, inv_h and n are an NmCells<3>'s fields, copied: as a member its padded
// 64 bytes would make this 144 bytes, not 136, and the workspace sizes are part of the interface.
struct NnGrid {
  double o[3];           // box minimum (origin of cell 0)
  double inv_h[3];       // cells per unit length (0 on a one-cell axis)
  double h[3];           // cell edge
  double hi[3];          // box maximum
  double slack[3];       // rounding allowance of the cell assignment (bounds are lowered by it)
  int n[3];              // cells per axis, n0 * n1 * n2 <= the cell budget
  int bad;               // the cloud holds a NaN / Inf coordinate in this item
};
static_assert(sizeof(NnGrid) == 136, "nm_nn_workspace depends on it");

static inline int nn_box_blocks(int p) {
  const int g = nm_div_up(p, kNnThreads * 8);
  return g < 1 ? 1 : (g > kBoxMaxBlocks ? kBoxMaxBlocks : g);
}
static inline int nn_mean_blocks(int p) {
  const int g = nm_div_up(p, kNnThreads * 16);
  return g < 1 ? 1 : (g > kMeanMaxBlocks ? kMeanMaxBlocks : g);
}
static inline int nn_cell_budget(int p) { return (int)(((int64_t)p + kPointsPerCell - 1) / kPointsPerCell); }

// One binned cloud (B items of P points): where its arrays live in the workspace.
struct NnBin {
  int b, p, cmax, gbox;
  NnBoxPart* part;
  NnGrid* grid;
  int* cnt;          // B * cmax + 1 counters
  int* start;        // their exclusive scan: first global sorted position of every cell, start[B * cmax] = B * P
  int* key;          // B * P
  int* rank;         // B * P
  float4* sorted;    // B * P
  NmIntScan scan;
};

static NnBin carve_bin(NmCarver& c, int b, int p) {
  NnBin w;
  w.b = b; w.p = p; w.cmax = nn_cell_budget(p); w.gbox = nn_box_blocks(p);
  const size_t np = (size_t)b * p, nc = (size_t)b * w.cmax + 1;
  w.part = c.take<NnBoxPart>((size_t)b * w.gbox);
  w.grid = c.take<NnGrid>(b);
  w.cnt = c.take<int>(nc);
  w.start = c.take<int>(nc);
  w.key = c.take<int>(np);          // key + rank: nm_chamfer may reuse the pair as B * P int64
  w.rank = c.take<int>(np);
  w.sorted = c.take<float4>(np);
  w.scan.carve(c, nc);
  return w;
}

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e+38f && fabsf(y) <= 3.402823466e+38f && fabsf(z) <= 3.402823466e+38f;
}

// grid (gbox, B): partial box of the finite points of item blockIdx.y, and the count of points with a non-finite coordinate
__global__ void __launch_bounds__(kNnThreads) k_nn_box(int P, int gbox, const float* __restrict__ pts, NnBoxPart* __restrict__ part) {
  constexpr int NW = kNnThreads / 64;
  __shared__ float red[NW * 6];
  __shared__ int rbad[NW];
  const int item = blockIdx.y;
  const float* X = pts + (size_t)item * P * 3;
  float bb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};      // lo[3], hi[3]
  int bad = 0;
  for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < P; i += gbox * kNnThreads) {
    const float x = X[3 * (size_t)i], y = X[3 * (size_t)i + 1], z = X[3 * (size_t)i + 2];
    if (nn_finite3(x, y, z)) {
      bb[0] = fminf(bb[0], x); bb[1] = fminf(bb[1], y); bb[2] = fminf(bb[2], z);
      bb[3] = fmaxf(bb[3], x); bb[4] = fmaxf(bb[4], y); bb[5] = fmaxf(bb[5], z);
    } else {
      ++bad;
    }
  }
  const auto tot = nm_block_reduce<NW, NmMinMax<3>>(bb, red);
  bad = nm_block_reduce<NW, NmSum>(bad, rbad);
  if (threadIdx.x == 0) {
    NnBoxPart r;
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.lo[k] = tot[k]; r.hi[k] = tot[3 + k]; }
    r.bad = bad;
    r.pad = 0;
    part[(size_t)item * gbox + blockIdx.x] = r;
  }
}

// one thread per item: the box, then its cells
__global__ void __launch_bounds__(64) k_nn_grid(int B, int gbox, int cmax, const NnBoxPart* __restrict__ part, NnGrid* __restrict__ grid) {
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item >= B) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, e[3];
  NnGrid G;
  G.bad = 0;
  for (int g = 0; g < gbox; ++g) {
    const NnBoxPart& r = part[(size_t)item * gbox + g];
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], (double)r.lo[k]); hi[k] = fmax(hi[k], (double)r.hi[k]); }
    G.bad += r.bad;
  }
  NmCells<3> c;
  nm_cells_fit(lo, hi, cmax, c, e);
  for (int k = 0; k < 3; ++k) {
    G.o[k] = c.o[k]; G.inv_h[k] = c.inv_h[k]; G.n[k] = c.n[k];
    G.hi[k] = hi[k];
    G.h[k] = e[k] / (double)G.n[k];
    G.slack[k] = 1e-9 * (fabs(G.o[k]) + fabs(G.hi[k])) + 1e-300;
  }
  grid[item] = G;
}

__device__ __forceinline__ int nn_key(const NnGrid& G, float x, float y, float z) {
  const int cx = nm_cell(x, G.o[0], G.inv_h[0], G.n[0]);
  const int cy = nm_cell(y, G.o[1], G.inv_h[1], G.n[1]);
  const int cz = nm_cell(z, G.o[2], G.inv_h[2], G.n[2]);
  return (cx * G.n[1] + cy) * G.n[2] + cz;
}

// grid (ceil(P / 256), B)
__global__ void __launch_bounds__(kNnThreads) k_nn_count(int P, int cmax, const float* __restrict__ pts, const NnGrid* __restrict__ grid,
                                                         int* __restrict__ cnt, int* __restrict__ key, int* __restrict__ rank) {
  const int i = blockIdx.x * kNnThreads + threadIdx.x;
  if (i >= P) return;
  const int item = blockIdx.y;
  const size_t gi = (size_t)item * P + i;
  const NnGrid& G = grid[item];
  const int k = nn_key(G, pts[3 * gi], pts[3 * gi + 1], pts[3 * gi + 2]);
  key[gi] = k;
  rank[gi] = atomicAdd(&cnt[(size_t)item * cmax + k], 1);
}

__global__ void __launch_bounds__(kNnThreads) k_nn_scatter(int P, int cmax, const float* __restrict__ pts, const int* __restrict__ start,
                                                           const int* __restrict__ key, const int* __restrict__ rank,
                                                           float4* __restrict__ sorted) {
  const int i = blockIdx.x * kNnThreads + threadIdx.x;
  if (i >= P) return;
  const int item = blockIdx.y;
  const size_t gi = (size_t)item * P + i;
  const int pos = start[(size_t)item * cmax + key[gi]] + rank[gi];
  sorted[pos] = make_float4(pts[3 * gi], pts[3 * gi + 1], pts[3 * gi + 2], __int_as_float(i));
}

// squared distance in fp64, summed x, y, z without contraction (cKDTree's order).  The pragma is what keeps the three products
// and the two sums separately rounded: HIP's __dmul_rn / __dadd_rn are plain * and + in a header, and the compiler fuses them
// into fmas under its default contraction.
__device__ __forceinline__ double nn_d2(double qx, double qy, double qz, const float4& t) {
#pragma clang fp contract(off)
  const double dx = qx - (double)t.x, dy = qy - (double)t.y, dz = qz - (double)t.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// What a search keeps per query: visit() offers one target, bound() is the squared distance beyond which no target can
// enter any more (the best for 1-NN, the k-th best for k-NN).
struct NnOne {
  double best = INFINITY;
  int bi = INT_MAX;
  __device__ __forceinline__ void visit(double d, int j) {
    if (d < best || (d == best && j < bi)) { best = d; bi = j; }
  }
  __device__ __forceinline__ double bound() const { return best; }
};

// The k best (distance^2, index) pairs in ascending lexicographic order, held in the LAST k of CAP >= k register slots: the
// first CAP - k slots hold (-inf, -1) sentinels that nothing ever moves, so the k-th best is always slot CAP - 1 and no slot is
// ever indexed by a run-time value.  Every loop over the slots is fully unrolled; the insertion is a compare-and-shift over all
// of them.
template <int CAP>
struct NnK {
  double d[CAP];
  int j[CAP];
  int skip;             // the target index that is no neighbour (exclude_same_index), -1 for none
  __device__ __forceinline__ NnK(int k, int skip_) : skip(skip_) {
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
      d[s] = s < CAP - k ? -INFINITY : INFINITY;
      j[s] = s < CAP - k ? -1 : INT_MAX;
    }
  }
  __device__ __forceinline__ static bool less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }
  __device__ __forceinline__ void visit(double dd, int jj) {
    if (jj == skip || !less(dd, jj, d[CAP - 1], j[CAP - 1])) return;
#pragma unroll
    for (int s = CAP - 1; s > 0; --s) {
      const bool before = less(dd, jj, d[s - 1], j[s - 1]);      // the newcomer goes in front of slot s - 1: slot s takes that one
      const bool here = !before && less(dd, jj, d[s], j[s]);
      d[s] = before ? d[s - 1] : (here ? dd : d[s]);
      j[s] = before ? j[s - 1] : (here ? jj : j[s]);
    }
    if (less(dd, jj, d[0], j[0])) { d[0] = dd; j[0] = jj; }
  }
  __device__ __forceinline__ double bound() const { return d[CAP - 1]; }
};

template <class Acc>
__device__ __forceinline__ void nn_scan_range(const float4* __restrict__ T, int s, int e, double qx, double qy, double qz, Acc& acc) {
  for (int k = s; k < e; ++k) {
    const float4 t = T[k];
    acc.visit(nn_d2(qx, qy, qz, t), __float_as_int(t.w));
  }
}

// squared distance from q to the interval [lo - s, hi + s] along one axis
__device__ __forceinline__ double nn_out2(double q, double lo, double hi, double s) {
  const double g = q < lo - s ? (lo - s) - q : (q > hi + s ? q - (hi + s) : 0.0);
  return g * g;
}

// The shell walk of one finite query over the targets' grid: growing shells of cells around the query's own (clamped) cell until
// acc.bound() is at most the lower bound on the squared distance to every unvisited cell, max(n) shells at the most.
template <class Acc>
__device__ __forceinline__ void nn_walk(const float4& q, const NnGrid& G, const int* __restrict__ S, const float4* __restrict__ tsorted,
                                        Acc& acc) {
  const double qv[3] = {(double)q.x, (double)q.y, (double)q.z};
  const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
  int c[3];
  double out2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = nm_cell(qv[k], G.o[k], G.inv_h[k], G.n[k]);
    out2[k] = nn_out2(qv[k], G.o[k], G.hi[k], G.slack[k]);
  }
  const int rmax = max(n0, max(n1, n2));
  for (int r = 0; r < rmax; ++r) {
    int lo[3], hi[3], plo[3], phi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = max(c[k] - r, 0); hi[k] = min(c[k] + r, G.n[k] - 1);
      plo[k] = max(c[k] - r + 1, 0); phi[k] = min(c[k] + r - 1, G.n[k] - 1);   // the block of shell r - 1 (empty at r = 0)
    }
    for (int x = lo[0]; x <= hi[0]; ++x) {
      const bool xin = r > 0 && x >= plo[0] && x <= phi[0];
      for (int y = lo[1]; y <= hi[1]; ++y) {
        const int base = (x * n1 + y) * n2;       // the cells of one (x, y) column are contiguous in the sorted cloud
        if (!(xin && y >= plo[1] && y <= phi[1])) {
          nn_scan_range(tsorted, S[base + lo[2]], S[base + hi[2] + 1], qv[0], qv[1], qv[2], acc);
        } else {
          if (lo[2] < plo[2]) nn_scan_range(tsorted, S[base + lo[2]], S[base + lo[2] + 1], qv[0], qv[1], qv[2], acc);
          if (hi[2] > phi[2]) nn_scan_range(tsorted, S[base + hi[2]], S[base + hi[2] + 1], qv[0], qv[1], qv[2], acc);
        }
      }
    }
    // lower bound on the squared distance to every unvisited cell: such a cell lies beyond one face of the block, inside the box
    double lb2 = INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double side = out2[(k + 1) % 3] + out2[(k + 2) % 3];
      if (lo[k] > 0) {
        const double g = fmax(qv[k] - (G.o[k] + lo[k] * G.h[k]) - G.slack[k], 0.0);
        lb2 = fmin(lb2, g * g + side);
      }
      if (hi[k] < G.n[k] - 1) {
        const double g = fmax((G.o[k] + (hi[k] + 1) * G.h[k]) - G.slack[k] - qv[k], 0.0);
        lb2 = fmin(lb2, g * g + side);
      }
    }
    if (acc.bound() <= lb2) break;
  }
}

// grid (ceil(N / 256), B): thread t takes the t-th query of the query cloud's cell order of item blockIdx.y
__global__ void __launch_bounds__(kNnThreads) k_nn_search(int N, int cmax_t, const float4* __restrict__ qsorted,
                                                          const NnGrid* __restrict__ tgrid, const int* __restrict__ tstart,
                                                          const float4* __restrict__ tsorted, int64_t* __restrict__ idx_out,
                                                          double* __restrict__ d2_out) {
  const int t = blockIdx.x * kNnThreads + threadIdx.x;
  if (t >= N) return;
  const int item = blockIdx.y;
  const float4 q = qsorted[(size_t)item * N + t];
  const int qi = __float_as_int(q.w);
  NnOne acc;
  if (nn_finite3(q.x, q.y, q.z)) nn_walk(q, tgrid[item], tstart + (size_t)item * cmax_t, tsorted, acc);
  const size_t o = (size_t)item * N + qi;
  idx_out[o] = acc.bi == INT_MAX ? 0 : (int64_t)acc.bi;
  if (d2_out) d2_out[o] = acc.bi == INT_MAX ? (double)NAN : acc.best;
}

// The same walk with a k-best list.  idx_out / d2_out (B, N, k), either may be NULL; mean_out (B, N) fp32 or NULL: the mean of
// the k squared distances, summed ascending in fp64 and rounded once.  A slot that found no target: index 0, distance NaN.
template <int CAP>
__global__ void __launch_bounds__(kNnThreads) k_nn_search_k(int N, int cmax_t, int k, int exclude_same, const float4* __restrict__ qsorted,
                                                            const NnGrid* __restrict__ tgrid, const int* __restrict__ tstart,
                                                            const float4* __restrict__ tsorted, int64_t* __restrict__ idx_out,
                                                            double* __restrict__ d2_out, float* __restrict__ mean_out) {
  const int t = blockIdx.x * kNnThreads + threadIdx.x;
  if (t >= N) return;
  const int item = blockIdx.y;
  const float4 q = qsorted[(size_t)item * N + t];
  const int qi = __float_as_int(q.w);
  NnK<CAP> acc(k, exclude_same ? qi : -1);
  if (nn_finite3(q.x, q.y, q.z)) nn_walk(q, tgrid[item], tstart + (size_t)item * cmax_t, tsorted, acc);
  const size_t row = (size_t)item * N + qi;
  const int off = CAP - k;                                  // slot s holds neighbour s - off
  double sum = 0.0;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    if (s >= off) {
      const bool found = acc.j[s] != INT_MAX;
      const double d = found ? acc.d[s] : (double)NAN;
      if (idx_out) idx_out[row * k + (s - off)] = found ? (int64_t)acc.j[s] : 0;
      if (d2_out) d2_out[row * k + (s - off)] = d;
      sum += d;
    }
  }
  if (mean_out) mean_out[row] = (float)(sum / (double)k);
}

// grid (gmean, B): fixed-order partial sums of d2 over the queries in their original order
__global__ void __launch_bounds__(kNnThreads) k_nn_mean_part(int N, int gmean, const double* __restrict__ d2, double* __restrict__ part) {
  __shared__ double red[kNnThreads / 64];
  const int item = blockIdx.y;
  const double* D = d2 + (size_t)item * N;
  double acc = 0.0;
  for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < N; i += gmean * kNnThreads) acc += D[i];
  acc = nm_block_reduce<kNnThreads / 64, NmSum>(acc, red);
  if (threadIdx.x == 0) part[(size_t)item * gmean + blockIdx.x] = acc;
}

// one workgroup: wave w finishes items w, w + 4, ...  mean = sum / N, NaN where either cloud of the item is non-finite
__global__ void __launch_bounds__(kNnThreads) k_nn_mean_finish(int B, int N, int gmean, const double* __restrict__ part,
                                                               const NnGrid* __restrict__ ga, const NnGrid* __restrict__ gb,
                                                               double* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int item = wave; item < B; item += kNnThreads / 64) {
    double acc = 0.0;
    for (int j = lane; j < gmean; j += 64) acc += part[(size_t)item * gmean + j];
    acc = nm_wave_reduce<NmSum>(acc);
    if (lane == 0) out[item] = (ga[item].bad || gb[item].bad) ? (double)NAN : acc / (double)N;
  }
}

static int nn_bin(const NnBin& w, const float* pts, hipStream_t s) {
  NM_LAUNCH(k_nn_box, dim3(w.gbox, w.b), dim3(kNnThreads), 0, s, w.p, w.gbox, pts, w.part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_nn_grid, dim3(nm_div_up(w.b, 64)), dim3(64), 0, s, w.b, w.gbox, w.cmax, (const NnBoxPart*)w.part, w.grid);
  NM_LAUNCH_CHECK();
  const size_t nc = (size_t)w.b * w.cmax + 1;
  NM_HIP_CHECK(hipMemsetAsync(w.cnt, 0, nc * sizeof(int), s));
  const dim3 pg(nm_div_up(w.p, kNnThreads), w.b);
  NM_LAUNCH(k_nn_count, pg, dim3(kNnThreads), 0, s, w.p, w.cmax, pts, (const NnGrid*)w.grid, w.cnt, w.key, w.rank);
  NM_LAUNCH_CHECK();
  if (int rc = w.scan.run(w.cnt, w.start, nc, s)) return rc;
  NM_LAUNCH(k_nn_scatter, pg, dim3(kNnThreads), 0, s, w.p, w.cmax, pts, (const int*)w.start, (const int*)w.key, (const int*)w.rank,
            w.sorted);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

static int nn_search(const NnBin& q, const NnBin& t, int64_t* idx, double* d2, hipStream_t s) {
  NM_LAUNCH(k_nn_search, dim3(nm_div_up(q.p, kNnThreads), q.b), dim3(kNnThreads), 0, s, q.p, t.cmax, (const float4*)q.sorted,
            (const NnGrid*)t.grid, (const int*)t.start, (const float4*)t.sorted, idx, d2);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

constexpr int kKnnMax = 16;

static int nn_search_k(const NnBin& q, const NnBin& t, int k, int exclude_same, int64_t* idx, double* d2, float* mean, hipStream_t s) {
  const dim3 g(nm_div_up(q.p, kNnThreads), q.b), b(kNnThreads);
  if (k <= 4) {
    NM_LAUNCH(k_nn_search_k<4>, g, b, 0, s, q.p, t.cmax, k, exclude_same, (const float4*)q.sorted, (const NnGrid*)t.grid,
              (const int*)t.start, (const float4*)t.sorted, idx, d2, mean);
  } else if (k <= 8) {
    NM_LAUNCH(k_nn_search_k<8>, g, b, 0, s, q.p, t.cmax, k, exclude_same, (const float4*)q.sorted, (const NnGrid*)t.grid,
              (const int*)t.start, (const float4*)t.sorted, idx, d2, mean);
  } else {
    NM_LAUNCH(k_nn_search_k<16>, g, b, 0, s, q.p, t.cmax, k, exclude_same, (const float4*)q.sorted, (const NnGrid*)t.grid,
              (const int*)t.start, (const float4*)t.sorted, idx, d2, mean);
  }
  NM_LAUNCH_CHECK();
  return NM_OK;
}

static int nn_mean(const NnBin& q, const NnBin& t, const double* d2, double* part, double* out, hipStream_t s) {
  const int gm = nn_mean_blocks(q.p);
  NM_LAUNCH(k_nn_mean_part, dim3(gm, q.b), dim3(kNnThreads), 0, s, q.p, gm, d2, part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_nn_mean_finish, dim3(1), dim3(kNnThreads), 0, s, q.b, q.p, gm, (const double*)part, (const NnGrid*)q.grid,
            (const NnGrid*)t.grid, out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

static bool nn_sizes_ok(int32_t b, int32_t n1, int32_t n2) {
  return b >= 1 && b <= 65535 && n1 >= 1 && n2 >= 1 && (int64_t)b * n1 < INT32_MAX && (int64_t)b * n2 < INT32_MAX;
}

struct ChamferWs {
  NnBin a, b;
  double *d2a, *d2b, *part;
};

static ChamferWs carve_chamfer(NmCarver& c, int b, int n1, int n2) {
  ChamferWs w;
  w.a = carve_bin(c, b, n1);
  w.b = carve_bin(c, b, n2);
  w.d2a = c.take<double>((size_t)b * n1);
  w.d2b = c.take<double>((size_t)b * n2);
  w.part = c.take<double>((size_t)b * (nn_mean_blocks(n1) + nn_mean_blocks(n2)));
  return w;
}

}  // namespace

extern "C" size_t nm_nn_workspace(int32_t b, int32_t n_query, int32_t n_target) {
  if (!nn_sizes_ok(b, n_query, n_target)) return 0;
  NmCarver c(nullptr);
  carve_bin(c, b, n_query);
  carve_bin(c, b, n_target);
  return c.total();
}

extern "C" int nm_nearest_neighbors(int32_t b, int32_t n_query, int32_t n_target, const float* query, const float* target,
                                    int64_t* idx_out, double* d2_out, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(b >= 1 && b <= 65535, "b must be in [1, 65535]");
  NM_REQUIRE(n_query >= 1 && n_target >= 1, "empty point cloud");
  NM_REQUIRE(nn_sizes_ok(b, n_query, n_target), "b * points above 2^31 - 1");
  NM_REQUIRE(query && target && idx_out && ws, "null pointer");
  NM_REQUIRE(ws_bytes >= nm_nn_workspace(b, n_query, n_target), "workspace too small (nm_nn_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  const NnBin q = carve_bin(c, b, n_query);
  const NnBin t = carve_bin(c, b, n_target);
  int rc;
  if ((rc = nn_bin(q, query, s)) != NM_OK) return rc;
  if ((rc = nn_bin(t, target, s)) != NM_OK) return rc;
  return nn_search(q, t, idx_out, d2_out, s);
}

extern "C" size_t nm_knn_workspace(int32_t b, int32_t n_query, int32_t n_target, int32_t k) {
  if (k < 1 || k > kKnnMax) return 0;
  return nm_nn_workspace(b, n_query, n_target);
}

extern "C" int nm_knn(int32_t b, int32_t n_query, int32_t n_target, int32_t k, int32_t exclude_same_index, const float* query,
                      const float* target, int64_t* idx_out, double* d2_out, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(k >= 1 && k <= kKnnMax, "k must be in [1, 16]");
  NM_REQUIRE(b >= 1 && b <= 65535, "b must be in [1, 65535]");
  NM_REQUIRE(n_query >= 1 && n_target >= 1, "empty point cloud");
  NM_REQUIRE(nn_sizes_ok(b, n_query, n_target), "b * points above 2^31 - 1");
  NM_REQUIRE((int64_t)b * n_query * k < INT32_MAX, "b * n_query * k above 2^31 - 1");
  NM_REQUIRE(n_target - (exclude_same_index ? 1 : 0) >= k, "fewer than k eligible targets");
  NM_REQUIRE(query && target && idx_out && ws, "null pointer");
  NM_REQUIRE(ws_bytes >= nm_knn_workspace(b, n_query, n_target, k), "workspace too small (nm_knn_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  const NnBin q = carve_bin(c, b, n_query);
  const NnBin t = carve_bin(c, b, n_target);
  int rc;
  if ((rc = nn_bin(q, query, s)) != NM_OK) return rc;
  if ((rc = nn_bin(t, target, s)) != NM_OK) return rc;
  return nn_search_k(q, t, k, exclude_same_index ? 1 : 0, idx_out, d2_out, nullptr, s);
}

extern "C" size_t nm_knn_mean_dist2_workspace(int32_t n) {
  if (!nn_sizes_ok(1, n, n)) return 0;
  NmCarver c(nullptr);
  carve_bin(c, 1, n);
  return c.total();
}

extern "C" int nm_knn_mean_dist2(int32_t n, const float* points, int32_t k, float* out, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(k >= 1 && k <= kKnnMax, "k must be in [1, 16]");
  NM_REQUIRE(n >= 1 && nn_sizes_ok(1, n, n), "bad point count");
  NM_REQUIRE(n - 1 >= k, "fewer than k other points");
  NM_REQUIRE(points && out && ws, "null pointer");
  NM_REQUIRE(ws_bytes >= nm_knn_mean_dist2_workspace(n), "workspace too small (nm_knn_mean_dist2_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  const NnBin cloud = carve_bin(c, 1, n);               // the cloud is binned once: it is both the queries and the targets
  int rc;
  if ((rc = nn_bin(cloud, points, s)) != NM_OK) return rc;
  return nn_search_k(cloud, cloud, k, 1, nullptr, nullptr, out, s);
}

extern "C" size_t nm_chamfer_workspace(int32_t b, int32_t n1, int32_t n2) {
  if (!nn_sizes_ok(b, n1, n2)) return 0;
  NmCarver c(nullptr);
  carve_chamfer(c, b, n1, n2);
  return c.total();
}

extern "C" int nm_chamfer(int32_t b, int32_t n1, int32_t n2, const float* p1, const float* p2, double* cd12_out, double* cd21_out,
                          int64_t* idx12, int64_t* idx21, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(b >= 1 && b <= 65535, "b must be in [1, 65535]");
  NM_REQUIRE(n1 >= 1 && n2 >= 1, "empty point cloud");
  NM_REQUIRE(nn_sizes_ok(b, n1, n2), "b * points above 2^31 - 1");
  NM_REQUIRE(p1 && p2 && cd12_out && cd21_out && ws, "null pointer");
  NM_REQUIRE(ws_bytes >= nm_chamfer_workspace(b, n1, n2), "workspace too small (nm_chamfer_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  const ChamferWs w = carve_chamfer(c, b, n1, n2);
  // without caller arrays the indices go to the (then unused) key arrays' space: B * n int64 = the key + rank arrays
  int64_t* i12 = idx12 ? idx12 : (int64_t*)w.a.key;
  int64_t* i21 = idx21 ? idx21 : (int64_t*)w.b.key;
  int rc;
  if ((rc = nn_bin(w.a, p1, s)) != NM_OK) return rc;
  if ((rc = nn_bin(w.b, p2, s)) != NM_OK) return rc;
  if ((rc = nn_search(w.a, w.b, i12, w.d2a, s)) != NM_OK) return rc;
  if ((rc = nn_search(w.b, w.a, i21, w.d2b, s)) != NM_OK) return rc;
  if ((rc = nn_mean(w.a, w.b, w.d2a, w.part, cd12_out, s)) != NM_OK) return rc;
  return nn_mean(w.b, w.a, w.d2b, w.part + (size_t)b * nn_mean_blocks(n1), cd21_out, s);
}
