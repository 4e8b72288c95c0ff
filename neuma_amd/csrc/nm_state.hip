// Particle-state loss of one frame (position + velocity, l1 or l2, optional row mask) fused with its gradient: the loss the
// constitutive pretraining loop (neuma_amd/pretrain.py) takes against a recorded trajectory.  No reference counterpart.
//   k_state_count   rows kept by the mask: one integer partial per workgroup (only launched with a mask)
//   k_state_loss    |d| or d^2 in fp64 over the flat (n,3) arrays, four floats per thread and iteration; gradients written
//                   already scaled by weight / (3 m); one fp64 partial per term and workgroup
//   k_state_finish  one workgroup: the partials in a fixed order, then *loss += weight_x term_x + weight_v term_v
// No float atomics anywhere: two calls give the same bits.  A thread owns the same four floats whether it loads them as one
// float4 (16-byte aligned bases) or one by one, and adds them in the same order, so both paths give the same bits too.
#include "nm_common.h"
#include "nm_reduce.h"

namespace {

constexpr int kStThreads = 256;
constexpr int kStMaxBlocks = 512;

static int state_blocks(int64_t items) {
  const int64_t b = (items + kStThreads - 1) / kStThreads;
  return b < 1 ? 1 : (b > kStMaxBlocks ? kStMaxBlocks : (int)b);
}
static size_t state_part_bytes() { return (size_t)kStMaxBlocks * 2 * sizeof(double); }

__global__ void __launch_bounds__(kStThreads) k_state_count(int n, const uint8_t* __restrict__ mask, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t sh[4];
  uint32_t c = 0;
  for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kStThreads) c += mask[i] != 0;
  c = nm_block_reduce<4, NmSum>(c, sh);
  if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

// rows kept: n without a mask, else the count partials (integers: exact in any order)
__device__ __forceinline__ uint32_t state_kept(int n, int nbc, const uint32_t* __restrict__ cnt, uint32_t* sh) {
  if (!cnt) return (uint32_t)n;
  return nm_block_sum_partials<4, 1>(cnt, nbc, 1, sh)[0];
}

// One of the two terms over `total` = 3 n floats.  Thread t of the grid owns floats [4 q, 4 q + 4) for q = t, t + grid, ...
// Returns this thread's unnormalised sum; grad (may be NULL) = scale * d|d|/da or scale * d(d^2)/da, 0 on masked-out rows.
template <bool VEC>
__device__ __forceinline__ double state_term(int64_t total, int kind, double scale, const float* __restrict__ a,
                                             const float* __restrict__ b, const uint8_t* __restrict__ mask,
                                             float* __restrict__ grad) {
  double acc = 0.0;
  const int64_t quads = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * kStThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kStThreads) {
    const int64_t e0 = q << 2;
    const bool full = total - e0 >= 4;
    float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f}, vg[4];
    if (VEC && full) {
      const float4 A = *reinterpret_cast<const float4*>(a + e0), B = *reinterpret_cast<const float4*>(b + e0);
      va[0] = A.x; va[1] = A.y; va[2] = A.z; va[3] = A.w;
      vb[0] = B.x; vb[1] = B.y; vb[2] = B.z; vb[3] = B.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k < total) { va[k] = a[e0 + k]; vb[k] = b[e0 + k]; }
    }
    int64_t row = e0 / 3;
    int rem = (int)(e0 - 3 * row);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = e0 + k < total;
      const bool keep = in && (mask ? mask[row] != 0 : true);
      const double d = (double)va[k] - (double)vb[k];
      const double t = kind == 1 ? d * d : fabs(d);
      const double gd = kind == 1 ? d + d : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
      if (keep) acc += t;
      vg[k] = keep ? (float)(scale * gd) : 0.f;
      if (++rem == 3) { rem = 0; ++row; }
    }
    if (grad) {
      if (VEC && full) {
        *reinterpret_cast<float4*>(grad + e0) = make_float4(vg[0], vg[1], vg[2], vg[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e0 + k < total) grad[e0 + k] = vg[k];
      }
    }
  }
  return acc;
}

__device__ __forceinline__ void state_zero(int64_t total, bool vec, float* __restrict__ grad) {
  const int64_t quads = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * kStThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kStThreads) {
    const int64_t e0 = q << 2;
    if (vec && total - e0 >= 4) {
      *reinterpret_cast<float4*>(grad + e0) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k < total) grad[e0 + k] = 0.f;
    }
  }
}

__global__ void __launch_bounds__(kStThreads) k_state_loss(int n, int kind, float wx, float wv, int vec_x, int vec_v,
                                                           const float* __restrict__ x, const float* __restrict__ v,
                                                           const float* __restrict__ x_gt, const float* __restrict__ v_gt,
                                                           const uint8_t* __restrict__ mask, int nbc,
                                                           const uint32_t* __restrict__ cnt, float* __restrict__ gx,
                                                           float* __restrict__ gv, double* __restrict__ part) {
  __shared__ uint32_t shc[4];
  __shared__ double shd[4];
  const uint32_t m = state_kept(n, nbc, cnt, shc);
  const double inv = m ? 1.0 / (3.0 * (double)m) : 0.0;
  const int64_t total = 3 * (int64_t)n;
  const double sx = (double)wx * inv;
  double ax = vec_x ? state_term<true>(total, kind, sx, x, x_gt, mask, gx) : state_term<false>(total, kind, sx, x, x_gt, mask, gx);
  double av = 0.0;
  if (v_gt) {
    const double sv = (double)wv * inv;
    av = vec_v ? state_term<true>(total, kind, sv, v, v_gt, mask, gv) : state_term<false>(total, kind, sv, v, v_gt, mask, gv);
  } else if (gv) {
    state_zero(total, vec_v != 0, gv);
  }
  ax = nm_block_reduce<4, NmSum>(ax, shd);
  av = nm_block_reduce<4, NmSum>(av, shd);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = ax;
    part[2 * blockIdx.x + 1] = av;
  }
}

__global__ void __launch_bounds__(kStThreads) k_state_finish(int n, int nb, const double* __restrict__ part, int nbc,
                                                             const uint32_t* __restrict__ cnt, float wx, float wv, int has_v,
                                                             float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ uint32_t shc[4];
  __shared__ double shd[4];
  const uint32_t m = state_kept(n, nbc, cnt, shc);
  const double ax = nm_block_sum_partials<4, 1>(part, nb, 2, shd)[0];
  const double av = nm_block_sum_partials<4, 1>(part + 1, nb, 2, shd)[0];
  if (threadIdx.x == 0) {
    const double inv = m ? 1.0 / (3.0 * (double)m) : 0.0;
    const double tx = ax * inv, tv = has_v ? av * inv : 0.0;
    if (m) *loss = (float)((double)*loss + ((double)wx * tx + (has_v ? (double)wv * tv : 0.0)));
    if (terms) {
      terms[0] = (float)tx;
      terms[1] = (float)tv;
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t nm_state_loss_workspace(int32_t n) {
  (void)n;      // both stages are capped at kStMaxBlocks workgroups whatever n
  return state_part_bytes() + (size_t)kStMaxBlocks * sizeof(uint32_t);
}

extern "C" int nm_state_loss(int32_t n, int32_t kind, float weight_x, float weight_v, const float* x, const float* v,
                             const float* x_gt, const float* v_gt, const uint8_t* mask, float* loss_out, float* terms_out,
                             float* dL_dx, float* dL_dv, void* workspace, size_t workspace_bytes, void* stream) {
  NM_REQUIRE(n >= 0, "n < 0");
  NM_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (l1) or 1 (l2)");
  if (n == 0) return NM_OK;
  NM_REQUIRE(x && x_gt && loss_out, "null pointer (x, x_gt, loss_out)");
  NM_REQUIRE(!v_gt || v, "v_gt given without v");
  NM_REQUIRE(workspace && workspace_bytes >= nm_state_loss_workspace(n), "workspace too small (nm_state_loss_workspace)");
  NM_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  double* part = (double*)workspace;
  uint32_t* cnt = mask ? (uint32_t*)((char*)workspace + state_part_bytes()) : nullptr;
  const int nbc = mask ? state_blocks(n) : 0;
  if (mask) {
    NM_LAUNCH(k_state_count, dim3(nbc), dim3(kStThreads), 0, (hipStream_t)stream, (int)n, mask, cnt);
    NM_LAUNCH_CHECK();
  }
  const int nb = state_blocks((3 * (int64_t)n + 3) / 4);
  const int vec_x = aligned16(x) && aligned16(x_gt) && aligned16(dL_dx);
  const int vec_v = v_gt ? (aligned16(v) && aligned16(v_gt) && aligned16(dL_dv)) : aligned16(dL_dv);
  NM_LAUNCH(k_state_loss, dim3(nb), dim3(kStThreads), 0, (hipStream_t)stream, (int)n, (int)kind, weight_x, weight_v, vec_x, vec_v,
            x, v, x_gt, v_gt, mask, nbc, (const uint32_t*)cnt, dL_dx, dL_dv, part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_state_finish, dim3(1), dim3(kStThreads), 0, (hipStream_t)stream, (int)n, nb, (const double*)part, nbc,
            (const uint32_t*)cnt, weight_x, weight_v, v_gt ? 1 : 0, loss_out, terms_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
