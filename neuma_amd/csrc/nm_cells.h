// What the files that bin things into a uniform grid share (nm_nn, nm_mesh, nm_bindbuild, nm_fill, nm_chamfer_loss):
//   NmCells<D>, nm_cells_fit   cells per axis of a box within a cell budget (host + device: tests/test_cells_host_cpu.py)
//   nm_cell                    the clamped, monotone map coordinate -> cell
//   k_nm_segment_starts        first sorted position of every segment (cell, block) from sorted keys
//   NmIntScan, NmSortPairs32   rocPRIM's exclusive int scan / 32-bit pair sort, temporary storage carved from an NmCarver
#pragma once
#include "nm_common.h"
#include "nm_workspace.h"

#include <math.h>
#include <rocprim/rocprim.hpp>

template <int D>
struct NmCells {
  double o[D];         // box minimum (origin of cell 0)
  double inv_h[D];     // cells per unit length (0 on a one-cell axis)
  int n[D];            // cells per axis, their product <= the cell budget
};

// Cells of the box [lo, hi] within a budget of cmax >= 1 cells; extent[k] = hi[k] - lo[k].  An axis with lo > hi (nothing
// finite went into the box) is rewritten to [0, 0].  An axis whose extent is zero or not finite gets one cell and inv_h = 0.
// Among the others, an axis shorter than the cubic cell edge h gets one cell and h is recomputed over the rest; then
// n_k = clamp(floor(e_k / h), 1, cmax), and the longest axis shrinks until the product is within the budget (the rounding of h).
template <int D>
__host__ __device__ inline void nm_cells_fit(double (&lo)[D], double (&hi)[D], int cmax, NmCells<D>& cells, double (&extent)[D]) {
  bool real[D], active[D];      // an extent that is positive and finite; of those, the axes still cut into cells of edge h
  for (int k = 0; k < D; ++k) {
    if (!(lo[k] <= hi[k])) { lo[k] = 0.0; hi[k] = 0.0; }
    cells.o[k] = lo[k];
    extent[k] = hi[k] - lo[k];
    real[k] = active[k] = extent[k] > 0.0 && extent[k] <= 1.7976931348623157e308;
  }
  double h = 0.0;
#pragma unroll 1      // (one copy of pow and sqrt: on the device this runs in one thread, and its time is its code size)
  for (int it = 0; it < D; ++it) {
    double a0 = 0.0, a1 = 0.0, vol = 1.0;        // the first two active extents, the product of all
    int d = 0;
    for (int k = 0; k < D; ++k)
      if (active[k]) {
        if (d == 0) a0 = extent[k];
        if (d == 1) a1 = extent[k];
        vol *= extent[k];
        ++d;
      }
    if (d == 0) break;
    if (d == 1) h = a0 / (double)cmax;
    else if (d == 2) h = sqrt(a0 / (double)cmax * a1);      // (the budget divides first: the extents' product may overflow)
    else h = pow(vol / (double)cmax, 1.0 / d);
    bool changed = false;
    for (int k = 0; k < D; ++k)
      if (active[k] && extent[k] < h) { active[k] = false; changed = true; }
    if (!changed) break;
  }
  for (int k = 0; k < D; ++k) {
    double nk = active[k] && h > 0.0 ? floor(extent[k] / h) : 1.0;
    nk = fmin(fmax(nk, 1.0), (double)cmax);
    cells.n[k] = (int)nk;
  }
  for (;;) {
    int64_t prod = 1;                            // (stops at the first factor that takes it over: never above cmax^2)
    int most = 0;
    for (int k = 0; k < D; ++k) {
      if (prod <= cmax) prod *= cells.n[k];
      most = cells.n[k] > most ? cells.n[k] : most;
    }
    if (prod <= cmax) break;
    for (int k = 0, done = 0; k < D; ++k)        // (the first of the longest axes; no index computed at run time)
      if (!done && cells.n[k] == most) { cells.n[k] -= most / 64 > 1 ? most / 64 : 1; done = 1; }
  }
  for (int k = 0; k < D; ++k) cells.inv_h[k] = real[k] ? (double)cells.n[k] / extent[k] : 0.0;
}

// the one monotone map from a coordinate to its cell (NaN -> 0, +-Inf -> an edge cell: every input lands in a cell of the grid)
__host__ __device__ __forceinline__ int nm_cell(double x, double o, double inv_h, int n) {
  double f = floor((x - o) * inv_h);
  f = fmin(fmax(f, 0.0), (double)(n - 1));
  return (int)f;
}

// how a sorted key names its segment
struct NmKeyItself {
  __device__ __forceinline__ uint32_t operator()(uint32_t key) const { return key; }
};
struct NmKeyHighWord {
  __device__ __forceinline__ uint32_t operator()(uint64_t key) const { return (uint32_t)(key >> 32); }
};

// grid ceil((n + 1) / 256): start[s] = first position in the n sorted keys of a key whose segment is >= s, for s in [0, nseg];
// start[nseg] = n.  A key's segment is clamped to nseg, so a key that names no segment writes nothing out of range; n = 0
// writes nseg + 1 zeros and reads no key.
template <class Key, class SegmentOf>
__global__ void __launch_bounds__(256) k_nm_segment_starts(long long n, int nseg, const Key* __restrict__ keys_sorted,
                                                           int* __restrict__ start) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const uint32_t ns = (uint32_t)nseg;
  uint32_t cur = ns, first = 0;                  // (both keys are loaded before either is clamped: one wait for the two)
  if (i < n) cur = SegmentOf()(keys_sorted[i]);
  if (i > 0) first = SegmentOf()(keys_sorted[i - 1]);
  cur = min(cur, ns);
  first = i > 0 ? min(first, ns) + 1 : 0;
  for (uint32_t s = first; s <= cur; ++s) start[s] = (int)i;
}

template <class SegmentOf, class Key>
static inline int nm_segment_starts(const Key* keys_sorted, int64_t n, int nseg, int* start, hipStream_t s) {
  const auto k_nm_segment_starts = ::k_nm_segment_starts<Key, SegmentOf>;      // (NM_LAUNCH's profile name: one word)
  NM_LAUNCH(k_nm_segment_starts, dim3(nm_div_up(n + 1, 256)), dim3(256), 0, s, (long long)n, nseg, keys_sorted, start);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

// bits of a radix sort whose keys are below n
static inline unsigned nm_key_bits(int64_t n) {
  unsigned bits = 1;
  while (((int64_t)1 << bits) < n) ++bits;
  return bits;
}

// rocPRIM's temporary size is asked for with null pointers and remembered; at least one byte is carved, so that the pointer
// is never one that rocPRIM takes for a size query.
struct NmIntScan {
  void* tmp = nullptr;
  size_t bytes = 0;
  // at_least: what another rocPRIM call that runs before or after the scan needs in the same region
  void carve(NmCarver& c, size_t n, size_t at_least = 0) {
    (void)rocprim::exclusive_scan(nullptr, bytes, (int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>(), (hipStream_t)0);
    bytes = bytes > at_least ? bytes : at_least;
    tmp = c.take<char>(bytes > 0 ? bytes : 1);
  }
  // out[i] = in[0] + ... + in[i - 1]
  int run(const int* in, int* out, size_t n, hipStream_t s) const {
    size_t tb = bytes;
    NM_HIP_CHECK(rocprim::exclusive_scan(tmp, tb, in, out, 0, n, rocprim::plus<int>(), s));
    return NM_OK;
  }
};

// a stable sort of (key, value) pairs of uint32_t: the four arrays of n_max elements and the temporary storage
struct NmSortPairs32 {
  uint32_t *key_in = nullptr, *key_out = nullptr, *val_in = nullptr, *val_out = nullptr;
  void* tmp = nullptr;
  size_t bytes = 0;
  void carve(NmCarver& c, size_t n_max) {
    key_in = c.take<uint32_t>(n_max); key_out = c.take<uint32_t>(n_max);
    val_in = c.take<uint32_t>(n_max); val_out = c.take<uint32_t>(n_max);
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n_max,
                                    0u, 32u, (hipStream_t)0);
    tmp = c.take<char>(bytes > 0 ? bytes : 1);
  }
  // the first n pairs of (key_in, val_in) by their keys' low `bits` bits into (key_out, val_out)
  int run(size_t n, unsigned bits, hipStream_t s) const {
    size_t tb = bytes;
    NM_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tb, key_in, key_out, val_in, val_out, n, 0u, bits, s));
    return NM_OK;
  }
};
