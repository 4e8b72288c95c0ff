// The per-Gaussian activations of a 3DGS parameter set and their adjoint, one thread per Gaussian (gaussian_model.py:26-41):
//   nm_gaussian_activate           (log-scales, raw quaternion, opacity logit) -> (cov6, opacity)
//   nm_gaussian_activate_backward  (dL/dcov6, dL/dopacity) -> (dL/dlog-scales, dL/dquaternion, dL/dlogit), overwritten
// The chain is the one nm_regist.hip runs behind its global transform (nm_gaussian.h).  Memory-bound: ~14 floats in and out per
// Gaussian, read and written with plain per-thread strides (a wave's lanes cover one contiguous stretch of every array, so each
// cache line it touches is used whole).
#include "nm_common.h"
#include "nm_gaussian.h"

namespace {

constexpr int kGaussThreads = 256;

struct GaussFwd {
  float e[3];      // scale_modifier * exp(log_scales)
  float q[4];      // rot / |rot|
  float len;       // |rot| (clamped)
  float M[9];      // build_rotation(q)
};

__device__ __forceinline__ void gauss_forward(int i, const float* __restrict__ ls, const float* __restrict__ rot, float mod, GaussFwd& f) {
#pragma unroll
  for (int a = 0; a < 3; ++a) f.e[a] = mod * expf(ls[3 * i + a]);
  const float4 r4 = reinterpret_cast<const float4*>(rot)[i];
  const float rq[4] = {r4.x, r4.y, r4.z, r4.w};
  f.len = qnormalize(rq, f.q);
  quat_rot(f.q, f.M);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void __launch_bounds__(kGaussThreads) k_gauss_activate(int K, const float* __restrict__ ls, const float* __restrict__ rot,
                                                                  const float* __restrict__ logit, float mod, float* __restrict__ cov6,
                                                                  float* __restrict__ opacity) {
  const int i = blockIdx.x * kGaussThreads + threadIdx.x;
  if (i >= K) return;
  if (cov6) {
    GaussFwd f;
    gauss_forward(i, ls, rot, mod, f);
    cov6_build(f.M, f.e, cov6, i);
  }
  if (opacity) opacity[i] = sigmoidf(logit[i]);
}

__global__ void __launch_bounds__(kGaussThreads) k_gauss_activate_bwd(int K, const float* __restrict__ ls, const float* __restrict__ rot,
                                                                      const float* __restrict__ logit, float mod,
                                                                      const float* __restrict__ gc, const float* __restrict__ gop,
                                                                      float* __restrict__ dls, float* __restrict__ drot,
                                                                      float* __restrict__ dlogit) {
  const int i = blockIdx.x * kGaussThreads + threadIdx.x;
  if (i >= K) return;
  if (gc) {
    GaussFwd f;
    gauss_forward(i, ls, rot, mod, f);
    const int o = 6 * i;
    const float g6[6] = {gc[o], gc[o + 1], gc[o + 2], gc[o + 3], gc[o + 4], gc[o + 5]};
    float dM[9], dl[3];
    cov6_adj(g6, f.M, f.e, dM, [&](int b, float de) { dl[b] = de * f.e[b]; });      // e = mod exp(ls): de/dls = e
    if (dls) {
#pragma unroll
      for (int a = 0; a < 3; ++a) dls[3 * i + a] = dl[a];
    }
    if (drot) {
      float dq[4], dr[4];
      quat_rot_adj(f.q, dM, dq);
      norm_adj(f.q, f.len, dq, dr);
      reinterpret_cast<float4*>(drot)[i] = make_float4(dr[0], dr[1], dr[2], dr[3]);
    }
  }
  if (gop) {
    const float s = sigmoidf(logit[i]);
    dlogit[i] = gop[i] * (s * (1.f - s));
  }
}

}  // namespace

extern "C" int nm_gaussian_activate(int32_t k, const float* log_scales, const float* rot, const float* opacity_logit,
                                    float scale_modifier, float* cov6, float* opacity, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  if (k == 0 || (!cov6 && !opacity)) return NM_OK;
  NM_REQUIRE(!cov6 || (log_scales && rot), "cov6 needs log_scales and rot");
  NM_REQUIRE(!opacity || opacity_logit, "opacity needs opacity_logit");
  NM_REQUIRE(!cov6 || (uintptr_t)rot % 16 == 0, "rot must be 16-byte aligned");
  NM_LAUNCH(k_gauss_activate, dim3(nm_div_up(k, kGaussThreads)), dim3(kGaussThreads), 0, (hipStream_t)stream, (int)k, log_scales, rot,
            opacity_logit, scale_modifier, cov6, opacity);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_gaussian_activate_backward(int32_t k, const float* log_scales, const float* rot, const float* opacity_logit,
                                             float scale_modifier, const float* dL_dcov6, const float* dL_dopacity,
                                             float* dL_dlog_scales, float* dL_drot, float* dL_dopacity_logit, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  const bool cov = dL_dlog_scales || dL_drot;
  NM_REQUIRE(!cov || (dL_dcov6 && log_scales && rot), "dL_dlog_scales / dL_drot need dL_dcov6, log_scales and rot");
  NM_REQUIRE(!dL_dopacity_logit || (dL_dopacity && opacity_logit), "dL_dopacity_logit needs dL_dopacity and opacity_logit");
  if (k == 0 || (!cov && !dL_dopacity_logit)) return NM_OK;
  NM_REQUIRE(!cov || ((uintptr_t)rot | (uintptr_t)dL_drot) % 16 == 0, "rot / dL_drot must be 16-byte aligned");
  NM_LAUNCH(k_gauss_activate_bwd, dim3(nm_div_up(k, kGaussThreads)), dim3(kGaussThreads), 0, (hipStream_t)stream, (int)k, log_scales,
            rot, opacity_logit, scale_modifier, cov ? dL_dcov6 : nullptr, dL_dopacity_logit ? dL_dopacity : nullptr, dL_dlog_scales,
            dL_drot, dL_dopacity_logit);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
