// nm_gaussian_deform: the raw 3DGS parameters (log-scales, quaternion) of K deformed Gaussians, one Gaussian per lane.  The
// per-Gaussian body is nm_gaussian_deform_one (nm_gaussian_deform.h): one 3x3 product, one nm_svd3, three logf, one quaternion.
// 92 B of traffic per Gaussian (12 + 16 + 36 in, 12 + 16 out) behind up to 5 Jacobi sweeps: latency-bound, no LDS, no atomics, no
// workspace.  Off the frame path: called once per exported frame (neuma_amd/export.py).
#include "nm_common.h"
#include "nm_gaussian_deform.h"

namespace {

constexpr int kDeformThreads = 256;

__global__ void __launch_bounds__(kDeformThreads) k_gaussian_deform(int K, const float* __restrict__ ls, const float* __restrict__ rot,
                                                                    const float* __restrict__ F, float mod, float* __restrict__ ls_out,
                                                                    float* __restrict__ rot_out) {
  const int i = blockIdx.x * kDeformThreads + threadIdx.x;
  if (i >= K) return;
  const float l[3] = {ls[3 * (size_t)i], ls[3 * (size_t)i + 1], ls[3 * (size_t)i + 2]};
  const float4 r4 = reinterpret_cast<const float4*>(rot)[i];
  const float rq[4] = {r4.x, r4.y, r4.z, r4.w};
  float Fm[9];      // (the identity is filled in here: a pointer chosen at run time would put the array into scratch memory)
#pragma unroll
  for (int a = 0; a < 9; ++a) Fm[a] = F ? F[9 * (size_t)i + a] : (a % 4 == 0 ? 1.f : 0.f);
  float lo[3], qo[4];
  nm_gaussian_deform_one(l, rq, Fm, mod, lo, qo);
#pragma unroll
  for (int a = 0; a < 3; ++a) ls_out[3 * (size_t)i + a] = lo[a];
  reinterpret_cast<float4*>(rot_out)[i] = make_float4(qo[0], qo[1], qo[2], qo[3]);
}

// [a, a + na) and [b, b + nb) floats share a byte
bool overlaps(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * na, b0 = (uintptr_t)b, b1 = b0 + 4 * nb;
  return a && b && a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int nm_gaussian_deform(int32_t k, const float* log_scales, const float* rot, const float* F, float scale_modifier,
                                  float* log_scales_out, float* rot_out, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(log_scales && rot && log_scales_out && rot_out, "log_scales, rot, log_scales_out and rot_out must not be NULL");
  NM_REQUIRE(((uintptr_t)rot | (uintptr_t)rot_out) % 16 == 0, "rot / rot_out must be 16-byte aligned");
  const size_t n = (size_t)k;
  const float* in[3] = {log_scales, rot, F};
  const size_t in_n[3] = {3 * n, 4 * n, 9 * n};
  for (int a = 0; a < 3; ++a)
    NM_REQUIRE(!overlaps(in[a], in_n[a], log_scales_out, 3 * n) && !overlaps(in[a], in_n[a], rot_out, 4 * n),
               "outputs must not overlap the inputs");
  NM_REQUIRE(!overlaps(log_scales_out, 3 * n, rot_out, 4 * n), "log_scales_out and rot_out overlap");
  NM_LAUNCH(k_gaussian_deform, dim3(nm_div_up(k, kDeformThreads)), dim3(kDeformThreads), 0, (hipStream_t)stream, (int)k, log_scales,
            rot, F, scale_modifier, log_scales_out, rot_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
