// Field paint (include/neuma_hip.h "field paint"): a per-particle quantity, its binding-weighted mean per Gaussian, the range of
// the finite values and the colour map, as SH DC coefficients the rasterizer takes as they are.
//   k_particle_field<Q>  one particle per lane, body nm_particle_field_one<Q> (nm_particle_field.h); one instantiation per quantity,
//                        each loading only what it reads into registers
//   k_field_range_*      min / max of the finite values: one reduction with two accumulators (nm_reduce.h), per-block partials, then
//                        one workgroup that also applies the widening rule or folds into the running pair
//   k_field_paint        one Gaussian per lane walks its CSR row; the knots travel by value in the kernel arguments
// All gather-bound and tiny next to a render: no LDS beyond the reductions' hand-over arrays, no atomics.  Off the training path.
#include "nm_common.h"
#include "nm_particle_field.h"
#include "nm_reduce.h"
#include "nm_workspace.h"

namespace {

constexpr int kPaintThreads = 256;
constexpr int kPaintWaves = kPaintThreads / 64;
constexpr int kRangeMaxBlocks = 1024;      // grid-stride above that: 1024 x 2 partials for the last workgroup

template <int Q>
__global__ void __launch_bounds__(kPaintThreads) k_particle_field(int n, const float* __restrict__ x, const float* __restrict__ v,
                                                                  const float* __restrict__ F, const float* __restrict__ stress,
                                                                  const float* __restrict__ x0, float* __restrict__ q_out) {
  const int i = blockIdx.x * kPaintThreads + threadIdx.x;
  if (i >= n) return;
  constexpr bool kX = Q == NM_FIELD_DISPLACEMENT, kV = Q == NM_FIELD_SPEED;
  constexpr bool kF = Q == NM_FIELD_VOLUME || Q == NM_FIELD_STRAIN || Q == NM_FIELD_PRESSURE || Q == NM_FIELD_VON_MISES;
  constexpr bool kS = Q == NM_FIELD_PRESSURE || Q == NM_FIELD_VON_MISES;
  // (every array is addressed through its own pointer, fixed at compile time per instantiation: a pointer picked at run time
  //  would put the matrices into scratch memory, see nm_export.hip)
  float xs[3] = {0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f}, x0s[3] = {0.f, 0.f, 0.f};
  M3 Fm = m3_ident(), Tm = m3_zero();
  if constexpr (kX) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { xs[a] = x[3 * (size_t)i + a]; x0s[a] = x0[3 * (size_t)i + a]; }
  }
  if constexpr (kV) {
#pragma unroll
    for (int a = 0; a < 3; ++a) vs[a] = v[3 * (size_t)i + a];
  }
  if constexpr (kF) Fm = m3_load(F + 9 * (size_t)i);
  if constexpr (kS) Tm = m3_load(stress + 9 * (size_t)i);
  q_out[i] = nm_particle_field_one<Q>(xs, vs, Fm, Tm, x0s);
}

// acc[0] by min, acc[1] by max; a non-finite value contributes to neither
__device__ __forceinline__ void range_take(float (&acc)[2], float g) {
  if (fabsf(g) <= 3.402823466e+38f) {
    acc[0] = fminf(acc[0], g);
    acc[1] = fmaxf(acc[1], g);
  }
}

__global__ void __launch_bounds__(kPaintThreads) k_field_range_partial(int k, const float* __restrict__ g, float* __restrict__ part) {
  __shared__ float sh[kPaintWaves * 2];
  float acc[2] = {INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * kPaintThreads + threadIdx.x; i < k; i += (int64_t)gridDim.x * kPaintThreads) range_take(acc, g[i]);
  const auto tot = nm_block_reduce<kPaintWaves, NmMinMax<1>>(acc, sh);
  if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = tot[threadIdx.x];
}

// one workgroup: the partials' min / max, then mode 0 (the frame's range, widened) or mode 1 (folded into the running pair)
__global__ void __launch_bounds__(kPaintThreads) k_field_range_final(int nb, const float* __restrict__ part, int mode,
                                                                     float* __restrict__ range) {
  __shared__ float sh[kPaintWaves * 2];
  float acc[2] = {INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < nb; b += kPaintThreads) {
    acc[0] = fminf(acc[0], part[2 * (size_t)b]);
    acc[1] = fmaxf(acc[1], part[2 * (size_t)b + 1]);
  }
  const auto tot = nm_block_reduce<kPaintWaves, NmMinMax<1>>(acc, sh);
  if (threadIdx.x == 0) {
    float lo = tot[0], hi = tot[1];
    if (mode == 0) {
      if (lo > hi) { lo = 0.f; hi = 1.f; }      // no finite value
      else if (!(hi > lo)) hi = lo + 1.f;       // a constant field
    } else {
      lo = fminf(lo, range[0]);
      hi = fmaxf(hi, range[1]);
    }
    range[0] = lo;
    range[1] = hi;
  }
}

__global__ void __launch_bounds__(kPaintThreads) k_field_paint(int K, int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ val, const float* __restrict__ q,
                                                               const float* __restrict__ range, NmPaintMap map, float* __restrict__ g_out,
                                                               float* __restrict__ dc_out) {
  const int i = blockIdx.x * kPaintThreads + threadIdx.x;
  if (i >= K) return;
  float g;
  if (rowptr) {
    const int b = rowptr[i], e = rowptr[i + 1];
    float num = 0.f, den = 0.f;
    bool bad = e <= b;
    for (int j = b; j < e; ++j) {
      const int c = col[j];
      const float w = val[j];
      const bool in = c >= 0 && c < n;
      const float qq = in ? q[c] : nm_field_nan();
      bad = bad || !(fabsf(qq) <= 3.402823466e+38f);
      num += w * qq;
      den += w;
    }
    g = (bad || den == 0.f) ? nm_field_nan() : num / den;
  } else {
    g = q[i];
  }
  if (g_out) g_out[i] = g;
  if (dc_out) {
    float dc[3];
    nm_field_color(g, range[0], range[1], map, dc);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dc_out[3 * (size_t)i + ch] = dc[ch];
  }
}

template <int Q>
void launch_field(int n, const float* x, const float* v, const float* F, const float* stress, const float* x0, float* q_out,
                  hipStream_t s) {
  NM_LAUNCH(k_particle_field<Q>, dim3(nm_div_up(n, kPaintThreads)), dim3(kPaintThreads), 0, s, n, x, v, F, stress, x0, q_out);
}

int range_blocks(int32_t k) { return k <= 0 ? 1 : (int)(nm_div_up(k, kPaintThreads) < kRangeMaxBlocks ? nm_div_up(k, kPaintThreads) : kRangeMaxBlocks); }

}  // namespace

extern "C" int nm_particle_field(int32_t n, int32_t quantity, const float* x, const float* v, const float* F, const float* stress,
                                 const float* x0, float* q_out, void* stream) {
  NM_REQUIRE(n >= 0, "n < 0");
  NM_REQUIREF(quantity >= 0 && quantity < NM_FIELD_COUNT, "unknown quantity %d", (int)quantity);
  if (n == 0) return NM_OK;
  NM_REQUIRE(q_out, "q_out must not be NULL");
  hipStream_t s = (hipStream_t)stream;
  switch (quantity) {
    case NM_FIELD_SPEED:
      NM_REQUIRE(v, "speed reads v: must not be NULL");
      launch_field<NM_FIELD_SPEED>(n, x, v, F, stress, x0, q_out, s);
      break;
    case NM_FIELD_DISPLACEMENT:
      NM_REQUIRE(x, "displacement reads x: must not be NULL");
      NM_REQUIRE(x0, "displacement reads x0: must not be NULL");
      launch_field<NM_FIELD_DISPLACEMENT>(n, x, v, F, stress, x0, q_out, s);
      break;
    case NM_FIELD_VOLUME:
      NM_REQUIRE(F, "volume reads F: must not be NULL");
      launch_field<NM_FIELD_VOLUME>(n, x, v, F, stress, x0, q_out, s);
      break;
    case NM_FIELD_STRAIN:
      NM_REQUIRE(F, "strain reads F: must not be NULL");
      launch_field<NM_FIELD_STRAIN>(n, x, v, F, stress, x0, q_out, s);
      break;
    case NM_FIELD_PRESSURE:
      NM_REQUIRE(F, "pressure reads F: must not be NULL");
      NM_REQUIRE(stress, "pressure reads stress: must not be NULL");
      launch_field<NM_FIELD_PRESSURE>(n, x, v, F, stress, x0, q_out, s);
      break;
    default:
      NM_REQUIRE(F, "von_mises reads F: must not be NULL");
      NM_REQUIRE(stress, "von_mises reads stress: must not be NULL");
      launch_field<NM_FIELD_VON_MISES>(n, x, v, F, stress, x0, q_out, s);
      break;
  }
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" size_t nm_field_range_workspace(int32_t k) {
  if (k < 0) return 0;
  NmCarver ws(nullptr);
  ws.take<float>(2 * (size_t)range_blocks(k));
  return ws.total();
}

extern "C" int nm_field_range(int32_t k, const float* g, float* range_inout, int32_t mode, void* workspace, size_t workspace_bytes,
                              void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  NM_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (frame range) or 1 (fold into the running range)");
  NM_REQUIRE(range_inout, "range_inout must not be NULL");
  NM_REQUIRE(k == 0 || g, "g must not be NULL");
  NM_REQUIRE(workspace && workspace_bytes >= nm_field_range_workspace(k), "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NmCarver ws(workspace);
  const int nb = range_blocks(k);
  float* part = ws.take<float>(2 * (size_t)nb);
  NM_LAUNCH(k_field_range_partial, dim3(nb), dim3(kPaintThreads), 0, s, (int)k, g, part);
  NM_LAUNCH(k_field_range_final, dim3(1), dim3(kPaintThreads), 0, s, nb, (const float*)part, (int)mode, range_inout);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_field_paint(int32_t k, int32_t n, const int32_t* rowptr, const int32_t* col, const float* val, const float* q,
                              const float* range_dev, int32_t n_knots, const float* knots, const float* nodata_rgb, float* g_out,
                              float* dc_out, void* stream) {
  NM_REQUIRE(k >= 0 && n >= 0, "k < 0 or n < 0");
  NM_REQUIRE(g_out || dc_out, "g_out and dc_out are both NULL: nothing to write");
  NM_REQUIRE(rowptr || k == n, "rowptr == NULL paints q itself: k must equal n");
  if (k == 0) return NM_OK;
  NM_REQUIRE(q || n == 0, "q must not be NULL");
  NM_REQUIRE(!rowptr || (col && val), "col and val must not be NULL with a rowptr");
  NmPaintMap map;
  memset(&map, 0, sizeof map);
  map.n = 2;
  if (dc_out) {
    NM_REQUIRE(range_dev, "range_dev must not be NULL with dc_out");
    NM_REQUIREF(n_knots >= 2 && n_knots <= NM_PAINT_MAX_KNOTS, "n_knots = %d outside 2..%d", (int)n_knots, NM_PAINT_MAX_KNOTS);
    NM_REQUIRE(knots && nodata_rgb, "knots and nodata_rgb must not be NULL with dc_out");
    map.n = n_knots;
    for (int a = 0; a < 3 * n_knots; ++a) map.c[a / 3][a % 3] = knots[a];
    for (int a = 0; a < 3; ++a) map.nodata[a] = nodata_rgb[a];
  }
  NM_LAUNCH(k_field_paint, dim3(nm_div_up(k, kPaintThreads)), dim3(kPaintThreads), 0, (hipStream_t)stream, (int)k, (int)n, rowptr, col, val,
            q, range_dev, map, g_out, dc_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
