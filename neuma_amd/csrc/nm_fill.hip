// Particles out of the Gaussians' own density field (data preparation; no reference counterpart: the reference sends its
// users to outside meshing tools for particles.ply).  neuma_amd/extras/gaussian_fill.py states the algorithm in numpy fp64
// and is the yardstick of everything here; neuma_amd/gaussian_fill.py is the caller.
//
//   density   d(c) = sum_k [m_k <= cutoff] o_k exp(-m_k / 2),  m_k = (c - mu_k)^T inv(Sigma_k) (c - mu_k), at the centre
//             c = lo + (i + 1/2) h of every lattice cell
//   classify  shell = d > tau; enclosed = not shell, and on each of the three axis lines through the cell a shell cell at a
//             strictly lower and one at a strictly higher index
//   emit      per kept cell, in ascending linear index (ix ny + iy) nz + iz, per_cell^3 points
//
// Density is a gather by block, not a scatter: K Gaussians adding into cells with float atomics would give sums that depend
// on arrival order, and the field has to be the same bytes on every run (the threshold turns its last bit into particles).
// The lattice is cut into blocks of 4 x 4 x 4 cells: 64 cells = one wave with one lane per cell, so a block's list is
// read once per wave and every lane keeps one running sum in a register.  8^3 blocks would share each list entry among
// eight cells per lane, but a Gaussian a cell or two wide - the common size once `resolution` is chosen to resolve them -
// would then be evaluated at 512 cells where it touches a few dozen.  Steps:
//   k_fill_gaussians   per Gaussian, fp64: inv(Sigma) by cofactors (as nm_bindbuild.hip), the blocks under the box of its
//                      cutoff ellipsoid, their count; a Gaussian with det <= 0 counts no block and is reported as skipped
//   exclusive scan of the counts (rocPRIM), k_fill_pairs writes the keys (block << 32) | k, radix sort of the keys
//                      (rocPRIM): every block's list is contiguous and in ascending Gaussian index, whatever order the
//                      pairs were written in
//   k_nm_segment_starts (nm_cells.h) first sorted position of every block, from the keys' high words
//   k_fill_density     one wave per block; its Gaussians (10 floats each: mu, the six entries of inv(Sigma), o) go through
//                      LDS NM_FILL_BATCH at a time, every lane adds its cell's terms in list order; a block with an empty
//                      list writes zeros, so the field needs no clear
// Classification is integer logic on the field: k_fill_lines (first / last shell index of every axis line),
// k_fill_classify (kind per cell + keep flag), an exclusive scan of the flags, k_fill_emit.
//
// Every index that comes from a float is clamped to the lattice before it addresses anything.  The file is compiled with
// -ffp-contract=off: the fp64 expressions (box, cell centre, emitted coordinate) must round as numpy's do.  The fp32 inner
// loop of k_fill_density alone opts back into contraction: its result is held to a tolerance, not to bits.
#include "nm_cells.h"

#define NM_FILL_BATCH 64
#define NM_FILL_BLOCK 4          // cells per block edge (4^3 = 64 = one wave)
#define NM_FILL_MAX_CELLS ((int64_t)1 << 27)

struct FillGrid {
  double o[3];     // low corner of cell (0,0,0)
  double h;        // cell edge
  int n[3];        // cells per axis
  int nb[3];       // blocks per axis
};

// cell coordinate of x (fp64), clamped to the lattice BEFORE the conversion to int
// (not nm_cell: it divides by h in fp64 and so rounds as numpy's lattice helper does)
__device__ __forceinline__ int fill_cell_coord(double x, double o, double h, int n) {
  double c = floor((x - o) / h);
  c = c < 0.0 ? 0.0 : c;                      // (NaN fails both comparisons and is caught by the next line)
  c = c <= (double)(n - 1) ? c : (double)(n - 1);
  return (int)c;
}

__global__ void __launch_bounds__(256) k_fill_gaussians(int K, FillGrid g, const float* __restrict__ means, const float* __restrict__ cov6,
                                                        const float* __restrict__ opacity, float cutoff, float* __restrict__ g10,
                                                        int* __restrict__ boxes, int* __restrict__ counts,
                                                        unsigned long long* __restrict__ totals) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double s00 = cov6[6 * k], s01 = cov6[6 * k + 1], s02 = cov6[6 * k + 2], s11 = cov6[6 * k + 3], s12 = cov6[6 * k + 4],
               s22 = cov6[6 * k + 5];
  // cofactors of the symmetric matrix; inv = cof / det
  const double c00 = s11 * s22 - s12 * s12, c01 = s12 * s02 - s01 * s22, c02 = s01 * s12 - s11 * s02;
  const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
  const double det = s00 * c00 + s01 * c01 + s02 * c02;
  float a[6] = {(float)(c00 / det), (float)(c01 / det), (float)(c02 / det), (float)(c11 / det), (float)(c12 / det), (float)(c22 / det)};
  bool ok = det > 0.0 && det <= 1.7976931348623157e308;
#pragma unroll
  for (int q = 0; q < 6; ++q) ok = ok && fabsf(a[q]) <= 3.402823466e+38f;
  const double mu[3] = {(double)means[3 * k], (double)means[3 * k + 1], (double)means[3 * k + 2]};
  const double sd[3] = {s00, s11, s22};
  int b0[3], b1[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const double v = (double)cutoff * sd[ax];
    const double e = sqrt(v > 0.0 ? v : 0.0) * 1.0001 + 1e-12;      // slightly inflated against the fp32 rounding of m
    b0[ax] = fill_cell_coord(mu[ax] - e, g.o[ax], g.h, g.n[ax]) / NM_FILL_BLOCK;
    b1[ax] = fill_cell_coord(mu[ax] + e, g.o[ax], g.h, g.n[ax]) / NM_FILL_BLOCK;
  }
  float* o = g10 + (size_t)10 * k;
  o[0] = means[3 * k]; o[1] = means[3 * k + 1]; o[2] = means[3 * k + 2];
#pragma unroll
  for (int q = 0; q < 6; ++q) o[3 + q] = ok ? a[q] : 0.f;
  o[9] = ok ? opacity[k] : 0.f;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) { boxes[6 * k + ax] = b0[ax]; boxes[6 * k + 3 + ax] = b1[ax]; }
  const int cnt = ok ? (b1[0] - b0[0] + 1) * (b1[1] - b0[1] + 1) * (b1[2] - b0[2] + 1) : 0;
  counts[k] = cnt;
  atomicAdd(&totals[0], (unsigned long long)cnt);        // (integer sums: the same on every run)
  if (!ok) atomicAdd(&totals[1], 1ull);
}

__global__ void __launch_bounds__(256) k_fill_pairs(int K, FillGrid g, const int* __restrict__ boxes, const int* __restrict__ counts,
                                                    const int* __restrict__ offsets, long long n_pairs, uint64_t* __restrict__ keys) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K || counts[k] == 0) return;
  long long at = offsets[k];
  // the box was clamped when it was written; clamp again, since it comes back through the caller's memory
  const int x0 = max(0, boxes[6 * k]), y0 = max(0, boxes[6 * k + 1]), z0 = max(0, boxes[6 * k + 2]);
  const int x1 = min(g.nb[0] - 1, boxes[6 * k + 3]), y1 = min(g.nb[1] - 1, boxes[6 * k + 4]), z1 = min(g.nb[2] - 1, boxes[6 * k + 5]);
  for (int bx = x0; bx <= x1; ++bx)
    for (int by = y0; by <= y1; ++by)
      for (int bz = z0; bz <= z1; ++bz) {
        if (at < 0 || at >= n_pairs) return;      // counts and n_pairs that do not belong together never write outside
        keys[at++] = ((uint64_t)(uint32_t)((bx * g.nb[1] + by) * g.nb[2] + bz) << 32) | (uint32_t)k;
      }
}

__global__ void __launch_bounds__(64) k_fill_density(int K, FillGrid g, const int* __restrict__ block_start,
                                                     const uint64_t* __restrict__ keys, const float* __restrict__ g10, float cutoff,
                                                     float* __restrict__ field) {
#pragma clang fp contract(fast)
  __shared__ float sg[NM_FILL_BATCH * 10];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int bz = b % g.nb[2], by = (b / g.nb[2]) % g.nb[1], bx = b / (g.nb[2] * g.nb[1]);
  const int ix = bx * NM_FILL_BLOCK + (lane >> 4), iy = by * NM_FILL_BLOCK + ((lane >> 2) & 3), iz = bz * NM_FILL_BLOCK + (lane & 3);
  const bool in = ix < g.n[0] && iy < g.n[1] && iz < g.n[2];      // blocks at the high faces may be partial
  // the cell centre: fp64, rounded to fp32 once
  const float cx = (float)(g.o[0] + ((double)ix + 0.5) * g.h);
  const float cy = (float)(g.o[1] + ((double)iy + 0.5) * g.h);
  const float cz = (float)(g.o[2] + ((double)iz + 0.5) * g.h);
  const int s0 = block_start[b], s1 = block_start[b + 1];
  float acc = 0.f;
  for (int base = s0; base < s1; base += NM_FILL_BATCH) {
    const int nb = min(NM_FILL_BATCH, s1 - base);
    __syncthreads();
    if (lane < nb) {
      const uint32_t k = (uint32_t)keys[base + lane];
      const bool ok = k < (uint32_t)K;
      const float* src = g10 + (size_t)10 * (ok ? k : 0u);
#pragma unroll
      for (int q = 0; q < 10; ++q) sg[lane * 10 + q] = ok ? src[q] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const float* G = sg + j * 10;
      const float dx = cx - G[0], dy = cy - G[1], dz = cz - G[2];
      const float m = dx * (G[3] * dx + 2.f * (G[4] * dy + G[5] * dz)) + dy * (G[6] * dy + 2.f * (G[7] * dz)) + G[8] * dz * dz;
      if (m <= cutoff) acc += G[9] * __expf(-0.5f * m);
    }
  }
  if (in) field[((size_t)ix * g.n[1] + iy) * g.n[2] + iz] = acc;
}

// ---------------------------------------------------------------- classification + emission

// one thread per axis line: first / last index of a shell cell on it (na / -1 when there is none).  The line runs along an
// axis of na cells with element stride sa; (cu, cv) = (line / nv, line % nv) names it, with strides su, sv.
__global__ void __launch_bounds__(256) k_fill_lines(int na, int nu, int nv, long long sa, long long su, long long sv,
                                                    const float* __restrict__ field, float tau, int* __restrict__ first,
                                                    int* __restrict__ last) {
  const int line = blockIdx.x * blockDim.x + threadIdx.x;
  if (line >= nu * nv) return;
  const float* p = field + (line / nv) * su + (line % nv) * sv;
  int f = na, l = -1;
  for (int i = 0; i < na; ++i)
    if (p[i * sa] > tau) { f = min(f, i); l = i; }
  first[line] = f;
  last[line] = l;
}

__global__ void __launch_bounds__(256) k_fill_classify(int n0, int n1, int n2, const float* __restrict__ field, float tau, int include_shell,
                                                       const int* __restrict__ fx, const int* __restrict__ lx, const int* __restrict__ fy,
                                                       const int* __restrict__ ly, const int* __restrict__ fz, const int* __restrict__ lz,
                                                       uint8_t* __restrict__ kind, int* __restrict__ keep, int* __restrict__ counts) {
  const long long ncells = (long long)n0 * n1 * n2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncells) return;
  const int iz = (int)(i % n2), iy = (int)((i / n2) % n1), ix = (int)(i / ((long long)n1 * n2));
  // line names as nm_fill_classify launches k_fill_lines: x lines by (iy, iz), y lines by (ix, iz), z lines by (ix, iy)
  const int px = iy * n2 + iz, py = ix * n2 + iz, pz = ix * n1 + iy;
  int kd;
  if (field[i] > tau) kd = 1;
  else kd = (fx[px] < ix && ix < lx[px] && fy[py] < iy && iy < ly[py] && fz[pz] < iz && iz < lz[pz]) ? 2 : 0;
  kind[i] = (uint8_t)kd;
  const int kp = kd == 2 || (kd == 1 && include_shell);
  keep[i] = kp;
  if (kp) atomicAdd(&counts[0], 1);
  if (kd == 1) atomicAdd(&counts[1], 1);
  if (kd == 2) atomicAdd(&counts[2], 1);
}

__global__ void __launch_bounds__(256) k_fill_emit(FillGrid g, int per_cell, int include_shell, const uint8_t* __restrict__ kind,
                                                   const int* __restrict__ offsets, long long n_kept, float* __restrict__ points,
                                                   uint8_t* __restrict__ kind_out) {
  const long long ncells = (long long)g.n[0] * g.n[1] * g.n[2];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncells) return;
  const int kd = kind[i];
  if (!(kd == 2 || (kd == 1 && include_shell))) return;
  const long long at = offsets[i];
  if (at < 0 || at >= n_kept) return;       // a count that does not belong to these offsets never writes outside
  const int c[3] = {(int)(i / ((long long)g.n[1] * g.n[2])), (int)((i / g.n[2]) % g.n[1]), (int)(i % g.n[2])};
  const int n = per_cell;
  size_t q = (size_t)at * n * n * n;
  for (int sx = 0; sx < n; ++sx)
    for (int sy = 0; sy < n; ++sy)
      for (int sz = 0; sz < n; ++sz, ++q) {
        const int s[3] = {sx, sy, sz};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)      // one fp64 expression, one rounding to fp32 (extras/gaussian_fill.py emit_points)
          points[3 * q + ax] = (float)(g.o[ax] + ((double)c[ax] + ((double)s[ax] + 0.5) / (double)n) * g.h);
        kind_out[q] = (uint8_t)kd;
      }
}

// ---------------------------------------------------------------- host side

static int fill_grid(FillGrid* g, const double* origin, double h, const int32_t* dims) {
  NM_REQUIRE(origin && dims, "null lattice");
  NM_REQUIRE(h > 0.0 && h <= 1.7976931348623157e308, "cell edge must be positive and finite");
  NM_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "lattice dims must be >= 1");
  NM_REQUIRE((int64_t)dims[0] * dims[1] * dims[2] <= NM_FILL_MAX_CELLS, "more than 2^27 lattice cells");
  for (int a = 0; a < 3; ++a) {
    NM_REQUIRE(origin[a] == origin[a] && origin[a] - origin[a] == 0.0, "lattice origin must be finite");
    g->o[a] = origin[a];
    g->n[a] = dims[a];
    g->nb[a] = (dims[a] + NM_FILL_BLOCK - 1) / NM_FILL_BLOCK;
  }
  g->h = h;
  return NM_OK;
}

extern "C" int nm_fill_gaussians(int32_t K, const float* means, const float* cov6, const float* opacity, const double* origin, double h,
                                 const int32_t* dims, float cutoff, float* g10, int32_t* boxes, int32_t* counts, int64_t* totals,
                                 void* stream) {
  NM_REQUIRE(K >= 1, "K must be >= 1");
  NM_REQUIRE(means && cov6 && opacity && g10 && boxes && counts && totals, "null pointer");
  NM_REQUIRE(cutoff > 0.f && cutoff <= 3.402823466e+38f, "cutoff must be positive and finite");
  FillGrid g;
  if (int rc = fill_grid(&g, origin, h, dims)) return rc;
  hipStream_t s = (hipStream_t)stream;
  NM_HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s));
  NM_LAUNCH(k_fill_gaussians, dim3(nm_div_up(K, 256)), dim3(256), 0, s, K, g, means, cov6, opacity, cutoff, g10, boxes, counts,
            (unsigned long long*)totals);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

struct FillWs { int* offsets; int* block_start; uint64_t *keys_in, *keys_out; NmIntScan scan; size_t total; };
static FillWs carve_fill_ws(void* base, int K, int64_t n_pairs, int nblocks) {
  FillWs w; NmCarver c(base);
  const size_t np = (size_t)(n_pairs > 0 ? n_pairs : 1);
  w.offsets = c.take<int>((size_t)K);
  w.block_start = c.take<int>((size_t)nblocks + 2);
  w.keys_in = c.take<uint64_t>(np);
  w.keys_out = c.take<uint64_t>(np);
  size_t sort_b = 0;      // the scan of the counts and the key sort run one after the other in one temporary region
  rocprim::radix_sort_keys(nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr, np, 0u, 64u, (hipStream_t)0);
  w.scan.carve(c, (size_t)K, sort_b);
  w.total = c.total();
  return w;
}

static bool fill_sizes_ok(int32_t K, int64_t n_pairs, int32_t nblocks) {
  return K >= 1 && n_pairs >= 0 && n_pairs <= 0x7fffffffLL && nblocks >= 1 && nblocks <= (int32_t)(NM_FILL_MAX_CELLS / 8);
}

extern "C" size_t nm_fill_density_workspace(int32_t K, int64_t n_pairs, int32_t n_blocks) {
  if (!fill_sizes_ok(K, n_pairs, n_blocks)) return 0;
  return carve_fill_ws(nullptr, K, n_pairs, n_blocks).total;
}

extern "C" int nm_fill_density(int32_t K, int64_t n_pairs, const float* g10, const int32_t* boxes, const int32_t* counts,
                               const double* origin, double h, const int32_t* dims, float cutoff, float* field, void* workspace,
                               size_t workspace_bytes, void* stream) {
  NM_REQUIRE(g10 && boxes && counts && field, "null pointer");
  FillGrid g;
  if (int rc = fill_grid(&g, origin, h, dims)) return rc;
  const int nblocks = g.nb[0] * g.nb[1] * g.nb[2];
  NM_REQUIRE(fill_sizes_ok(K, n_pairs, nblocks), "K must be >= 1 and the (Gaussian, block) pair count in [0, 2^31)");
  FillWs w = carve_fill_ws(workspace, K, n_pairs, nblocks);
  if (!workspace || workspace_bytes < w.total) {
    nm_set_error("fill workspace too small: need %zu got %zu", w.total, workspace_bytes);
    return NM_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = w.scan.run(counts, w.offsets, (size_t)K, s)) return rc;
  const uint64_t* sorted = w.keys_in;
  if (n_pairs > 0) {
    NM_LAUNCH(k_fill_pairs, dim3(nm_div_up(K, 256)), dim3(256), 0, s, K, g, boxes, counts, (const int*)w.offsets, (long long)n_pairs,
              w.keys_in);
    NM_LAUNCH_CHECK();
    size_t tb = w.scan.bytes;
    NM_HIP_CHECK(rocprim::radix_sort_keys(w.scan.tmp, tb, w.keys_in, w.keys_out, (size_t)n_pairs, 0u, 32u + nm_key_bits(nblocks), s));
    sorted = w.keys_out;
  }
  if (int rc = nm_segment_starts<NmKeyHighWord>(sorted, n_pairs, nblocks, w.block_start, s)) return rc;
  NM_LAUNCH(k_fill_density, dim3(nblocks), dim3(64), 0, s, K, g, (const int*)w.block_start, sorted, g10, cutoff, field);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

struct FillCws { int *first[3], *last[3]; int* keep; NmIntScan scan; size_t total; };
static FillCws carve_fill_cws(void* base, const int32_t* dims) {
  FillCws w; NmCarver c(base);
  const size_t nc = (size_t)dims[0] * dims[1] * dims[2];
  for (int a = 0; a < 3; ++a) {
    const size_t lines = nc / (size_t)dims[a];
    w.first[a] = c.take<int>(lines);
    w.last[a] = c.take<int>(lines);
  }
  w.keep = c.take<int>(nc);
  w.scan.carve(c, nc);
  w.total = c.total();
  return w;
}

static bool fill_dims_ok(const int32_t* dims) {
  return dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (int64_t)dims[0] * dims[1] * dims[2] <= NM_FILL_MAX_CELLS;
}

extern "C" size_t nm_fill_classify_workspace(const int32_t* dims) {
  if (!fill_dims_ok(dims)) return 0;
  return carve_fill_cws(nullptr, dims).total;
}

extern "C" int nm_fill_classify(const int32_t* dims, const float* field, float density_thres, int32_t include_shell, uint8_t* kind_cell,
                                int32_t* offsets, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  NM_REQUIRE(fill_dims_ok(dims), "lattice dims must be >= 1 and hold at most 2^27 cells");
  NM_REQUIRE(field && kind_cell && offsets && counts, "null pointer");
  FillCws w = carve_fill_cws(workspace, dims);
  if (!workspace || workspace_bytes < w.total) {
    nm_set_error("fill classify workspace too small: need %zu got %zu", w.total, workspace_bytes);
    return NM_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t nc = (size_t)dims[0] * dims[1] * dims[2];
  NM_HIP_CHECK(hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), s));
  const long long st[3] = {(long long)dims[1] * dims[2], (long long)dims[2], 1};
  for (int a = 0; a < 3; ++a) {
    const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;      // the two other axes, in ascending order
    NM_LAUNCH(k_fill_lines, dim3(nm_div_up((int64_t)dims[u] * dims[v], 256)), dim3(256), 0, s, dims[a], dims[u], dims[v], st[a], st[u],
              st[v], field, density_thres, w.first[a], w.last[a]);
    NM_LAUNCH_CHECK();
  }
  NM_LAUNCH(k_fill_classify, dim3(nm_div_up((int64_t)nc, 256)), dim3(256), 0, s, dims[0], dims[1], dims[2], field, density_thres,
            include_shell ? 1 : 0, (const int*)w.first[0], (const int*)w.last[0], (const int*)w.first[1], (const int*)w.last[1],
            (const int*)w.first[2], (const int*)w.last[2], kind_cell, w.keep, counts);
  NM_LAUNCH_CHECK();
  return w.scan.run(w.keep, offsets, nc, s);
}

extern "C" int nm_fill_emit(const int32_t* dims, const double* origin, double h, int32_t per_cell, int32_t include_shell,
                            const uint8_t* kind_cell, const int32_t* offsets, int64_t n_kept, float* points, uint8_t* kind_out,
                            void* stream) {
  NM_REQUIRE(per_cell >= 1 && per_cell <= 64, "per_cell must be in [1, 64]");
  NM_REQUIRE(n_kept >= 0 && n_kept <= NM_FILL_MAX_CELLS, "n_kept out of range");
  FillGrid g;
  if (int rc = fill_grid(&g, origin, h, dims)) return rc;
  if (n_kept == 0) return NM_OK;
  NM_REQUIRE(kind_cell && offsets && points && kind_out, "null pointer");
  const int64_t nc = (int64_t)dims[0] * dims[1] * dims[2];
  NM_LAUNCH(k_fill_emit, dim3(nm_div_up(nc, 256)), dim3(256), 0, (hipStream_t)stream, g, per_cell, include_shell ? 1 : 0, kind_cell, offsets,
            (long long)n_kept, points, kind_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
