// Classical constitutive laws (material/classical.py): the closed-form elasticity / plasticity presets of the reference's
// nclaw/material/preset.py:30-282 as one forward and one adjoint kernel per law, one thread per particle.
//   nm_classical_fwd   F (n,3,3), scalars {log_E, nu, p2, p3} on the device -> out (n,3,3)          36 B in, 36 B out
//   nm_classical_bwd   F, grad_out -> grad_F and {d/d log_E, d/d p2}: the SVD is recomputed; the scalar gradients are summed as
//                      fp64 per-block partials and one fixed-order block (as k_regist_bwd / k_regist_reduce): no atomics
// All arithmetic in registers, no LDS in the forward pass.  The SVD and its clamped adjoint are nm_common.h's (the ones behind
// nm_svd3_fwd / nm_svd3_bwd).  Every `where` of the reference is a select of two evaluated values; IEEE division and
// logf / expf / cbrtf throughout (no fast-math), so a NaN the reference produces is a NaN here.
#include "nm_common.h"
#include "nm_reduce.h"

namespace {

constexpr int kClThreads = 256;
constexpr int kClMaxBlocks = 1024;      // backward: grid-stride above 262 144 particles, so the partials stay a small array
constexpr float kSigmaMin = 0.05f;      // preset.py:214 / :262 ("prevent NaN")

struct ClParams {
  float mu, la, E, nu, p2, p3;
};

template <int LAW>
__device__ __forceinline__ ClParams cl_params(const float* __restrict__ sc) {
  ClParams P = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (LAW == NM_LAW_SIGMA_PLASTIC) return P;
  P.E = expf(sc[0]);
  P.nu = sc[1];
  P.mu = P.E / (2.f * (1.f + P.nu));
  P.la = P.E * P.nu / ((1.f + P.nu) * (1.f - 2.f * P.nu));
  if (LAW == NM_LAW_VON_MISES || LAW == NM_LAW_DRUCKER_PRAGER) P.p2 = sc[2];
  if (LAW == NM_LAW_DRUCKER_PRAGER) P.p3 = sc[3];
  return P;
}

// U diag(d) W^T
__device__ __forceinline__ M3 cl_udw(const M3& U, const float d[3], const M3& W) {
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o.m[3 * r + c] = U.m[3 * r] * d[0] * W.m[3 * c] + U.m[3 * r + 1] * d[1] * W.m[3 * c + 1] + U.m[3 * r + 2] * d[2] * W.m[3 * c + 2];
  return o;
}

// Hencky strain of the clamped singular values: eps = log max(sigma, 0.05), its trace, deviator and the deviator's norm
struct ClHencky {
  float eps[3], eh[3], tr, n;
};
__device__ __forceinline__ ClHencky cl_hencky(const float s[3]) {
  ClHencky h;
#pragma unroll
  for (int i = 0; i < 3; ++i) h.eps[i] = logf(fmaxf(s[i], kSigmaMin));
  h.tr = h.eps[0] + h.eps[1] + h.eps[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) h.eh[i] = h.eps[i] - h.tr / 3.f;
  h.n = sqrtf(h.eh[0] * h.eh[0] + h.eh[1] * h.eh[1] + h.eh[2] * h.eh[2]);
  return h;
}

// Drucker-Prager: alpha(friction angle in degrees), preset.py:251-252
constexpr float kSqrt23 = 0.816496580927726f;
constexpr float kDeg = 0.017453292519943295f;
__device__ __forceinline__ float cl_dp_alpha(float fa) {
  const float sp = sinf(fa * kDeg);
  return kSqrt23 * 2.f * sp / (3.f - sp);
}

// diagonal of the von Mises return map (yield side) / of the Drucker-Prager map; `yield` is the law's switch
__device__ __forceinline__ bool cl_von_mises(const ClHencky& h, const ClParams& P, float d[3]) {
  const float dg = h.n - P.p2 / (2.f * P.mu);
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = expf(h.eps[i] - (dg / h.n) * h.eh[i]);
  return dg > 0.f;
}
__device__ __forceinline__ bool cl_drucker_prager(const ClHencky& h, const ClParams& P, float d[3], float& q, bool& moved) {
  const float alpha = cl_dp_alpha(P.p2);
  const float sh = h.tr - P.p3 * 3.f;
  const bool yield = sh < 0.f;
  q = (3.f * P.la + 2.f * P.mu) / (2.f * P.mu) * sh * alpha;
  const float dgam = h.n + q;
  moved = dgam > 0.f;
  const float m = fmaxf(dgam, 0.f);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float ce = h.eps[i] - (m / h.n) * h.eh[i];      // (0 / 0 and inf * 0 give NaN here exactly where the reference's do)
    d[i] = expf(yield ? ce : P.p3);
  }
  return yield;
}

__device__ __forceinline__ float cl_volume_pressure(int mode, const ClParams& P, float J) {
  if (mode == NM_VOLUME_ZIRAN) return (2.f / 3.f * P.mu + P.la) * (J - 1.f / J);      // gamma = 2
  return P.la * J * (J - 1.f);
}

__device__ __forceinline__ float cl_cbrt(float J) { return J < 0.f ? __builtin_nanf("") : cbrtf(J); }      // torch.pow(J, 1/3)

template <int LAW>
__device__ __forceinline__ M3 cl_forward(const M3& F, const ClParams& P, int mode) {
  M3 out;
  if (LAW == NM_LAW_VOLUME) {
    out = m3_zero();
    out.m[0] = out.m[4] = out.m[8] = cl_volume_pressure(mode, P, m3_det(F));
    return out;
  }
  if (LAW == NM_LAW_SIGMA_PLASTIC) {
    out = m3_zero();
    out.m[0] = out.m[4] = out.m[8] = cl_cbrt(m3_det(F));
    return out;
  }
  M3 U, V;
  float s[3];
  nm_svd3(F, U, s, V);
  if (LAW == NM_LAW_COROTATED || LAW == NM_LAW_STVK) {
    const float J = s[0] * s[1] * s[2];
    const float vol = P.la * J * (J - 1.f);
    if (LAW == NM_LAW_COROTATED) {
      const M3 R = m3_mul_nt(U, V);
      M3 D;
#pragma unroll
      for (int i = 0; i < 9; ++i) D.m[i] = F.m[i] - R.m[i];
      out = m3_mul_nt(D, F);
#pragma unroll
      for (int i = 0; i < 9; ++i) out.m[i] *= 2.f * P.mu;
    } else {
      M3 C = m3_mul_tn(F, F);
      C.m[0] -= 1.f; C.m[4] -= 1.f; C.m[8] -= 1.f;
      out = m3_mul(F, C);
#pragma unroll
      for (int i = 0; i < 9; ++i) out.m[i] *= P.mu;      // 2 mu F (1/2 (F^T F - I))
    }
    out.m[0] += vol; out.m[4] += vol; out.m[8] += vol;
    return out;
  }
  if (LAW == NM_LAW_SIGMA) {
    float eps[3], tau[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) eps[i] = logf(s[i]);
    const float tr = eps[0] + eps[1] + eps[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) tau[i] = 2.f * P.mu * eps[i] + P.la * tr;
    return cl_udw(U, tau, U);
  }
  const ClHencky h = cl_hencky(s);
  float d[3];
  if (LAW == NM_LAW_VON_MISES) {
    const bool yield = cl_von_mises(h, P, d);
    const M3 Y = cl_udw(U, d, V);
#pragma unroll
    for (int i = 0; i < 9; ++i) out.m[i] = yield ? Y.m[i] : F.m[i];
    return out;
  }
  float q;
  bool moved;
  cl_drucker_prager(h, P, d, q, moved);
  return cl_udw(U, d, V);
}

// gs_i of a gradient on eps_i = log max(s_i, 0.05)
__device__ __forceinline__ void cl_eps_to_sigma(const float s[3], const float ge[3], float gs[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) gs[i] = s[i] > kSigmaMin ? ge[i] / s[i] : 0.f;
}

// adjoint of out = U diag(d) V^T given gd -> gs already mapped: gU = G V diag(d), gVh = diag(d) U^T G
__device__ __forceinline__ M3 cl_udv_adjoint(const M3& U, const float s[3], const M3& V, const M3& G, const float d[3],
                                             const float gs[3]) {
  M3 gU = m3_mul(G, V), gVh = m3_mul_tn(U, G);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) { gU.m[3 * r + c] *= d[c]; gVh.m[3 * r + c] *= d[r]; }
  return nm_svd3_adj(U, s, m3_transpose(V), gU, gs, gVh);
}

// one particle's adjoint; a0 / a1: its contribution to d/d log_E and d/d p2
template <int LAW>
__device__ __forceinline__ M3 cl_backward(const M3& F, const M3& G, const ClParams& P, int mode, float& a0, float& a1) {
  M3 gF;
  a0 = 0.f; a1 = 0.f;
  const float trG = G.m[0] + G.m[4] + G.m[8];
  if (LAW == NM_LAW_VOLUME) {
    const float J = m3_det(F);
    const float dp = mode == NM_VOLUME_ZIRAN ? (2.f / 3.f * P.mu + P.la) * (1.f + 1.f / (J * J)) : P.la * (2.f * J - 1.f);
    const M3 cof = m3_cofactor(F);
#pragma unroll
    for (int i = 0; i < 9; ++i) gF.m[i] = trG * dp * cof.m[i];
    a0 = trG * cl_volume_pressure(mode, P, J);      // the stress is linear in E = exp(log_E)
    return gF;
  }
  if (LAW == NM_LAW_SIGMA_PLASTIC) {
    const float J = m3_det(F);
    const float k = trG * cl_cbrt(J) / (3.f * J);
    const M3 cof = m3_cofactor(F);
#pragma unroll
    for (int i = 0; i < 9; ++i) gF.m[i] = k * cof.m[i];
    return gF;
  }
  M3 U, V;
  float s[3];
  nm_svd3(F, U, s, V);
  if (LAW == NM_LAW_COROTATED || LAW == NM_LAW_STVK) {
    const float J = s[0] * s[1] * s[2];
    const float gJ = P.la * (2.f * J - 1.f) * trG;
    const float gs[3] = {gJ * s[1] * s[2], gJ * s[0] * s[2], gJ * s[0] * s[1]};
    a0 = P.la * J * (J - 1.f) * trG;
    if (LAW == NM_LAW_COROTATED) {
      // out = 2 mu (F F^T - R F^T), R = U V^T:  direct 2 mu ((G + G^T) F - G^T R), through R: gR = -2 mu G F
      const M3 R = m3_mul_nt(U, V);
      M3 gR = m3_mul(G, F);
#pragma unroll
      for (int i = 0; i < 9; ++i) gR.m[i] *= -2.f * P.mu;
      gF = nm_svd3_adj(U, s, m3_transpose(V), m3_mul(gR, V), gs, m3_mul_tn(U, gR));
      M3 Gs;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Gs.m[3 * r + c] = G.m[3 * r + c] + G.m[3 * c + r];
      const M3 GsF = m3_mul(Gs, F), GtR = m3_mul_tn(G, R);
      M3 D;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        gF.m[i] += 2.f * P.mu * (GsF.m[i] - GtR.m[i]);
        D.m[i] = F.m[i] - R.m[i];
      }
      const M3 S = m3_mul_nt(D, F);
#pragma unroll
      for (int i = 0; i < 9; ++i) a0 += 2.f * P.mu * S.m[i] * G.m[i];
    } else {
      // out = mu F C, C = F^T F - I:  mu (G C + F (H + H^T)), H = F^T G
      M3 C = m3_mul_tn(F, F);
      C.m[0] -= 1.f; C.m[4] -= 1.f; C.m[8] -= 1.f;
      const M3 H = m3_mul_tn(F, G);
      M3 Hs;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Hs.m[3 * r + c] = H.m[3 * r + c] + H.m[3 * c + r];
      const M3 GC = m3_mul(G, C), FH = m3_mul(F, Hs), Jp = cl_udw(U, gs, V), S = m3_mul(F, C);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        gF.m[i] = P.mu * (GC.m[i] + FH.m[i]) + Jp.m[i];
        a0 += P.mu * S.m[i] * G.m[i];
      }
    }
    return gF;
  }
  if (LAW == NM_LAW_SIGMA) {
    float eps[3], tau[3], gt[3], ge[3], gs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) eps[i] = logf(s[i]);
    const float tr = eps[0] + eps[1] + eps[2];
    const M3 UtG = m3_mul_tn(U, G);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      tau[i] = 2.f * P.mu * eps[i] + P.la * tr;
      gt[i] = UtG.m[3 * i] * U.m[i] + UtG.m[3 * i + 1] * U.m[3 + i] + UtG.m[3 * i + 2] * U.m[6 + i];      // (U^T G U)_ii
      a0 += gt[i] * tau[i];
    }
    const float gsum = gt[0] + gt[1] + gt[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ge[i] = 2.f * P.mu * gt[i] + P.la * gsum; gs[i] = ge[i] / s[i]; }
    // out = U diag(tau) U^T: gU = (G + G^T) U diag(tau), no V
    M3 Gs;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Gs.m[3 * r + c] = G.m[3 * r + c] + G.m[3 * c + r];
    M3 gU = m3_mul(Gs, U);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) gU.m[3 * r + c] *= tau[c];
    return nm_svd3_adj(U, s, m3_transpose(V), gU, gs, m3_zero());
  }
  // the two plastic return maps: out = U diag(d) V^T, d = exp(e(eps))
  const ClHencky h = cl_hencky(s);
  const M3 UtG = m3_mul_tn(U, G);
  float d[3], ge[3], nh[3], geps[3], gs[3];
  if (LAW == NM_LAW_VON_MISES) {
    // yield side: e_i = tr / 3 + c eh_i / n with c = sigma_y / (2 mu)
    const bool yield = cl_von_mises(h, P, d);
    const float c = P.p2 / (2.f * P.mu);
    float dot = 0.f, gsum = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ge[i] = (UtG.m[3 * i] * V.m[i] + UtG.m[3 * i + 1] * V.m[3 + i] + UtG.m[3 * i + 2] * V.m[6 + i]) * d[i];      // (U^T G V)_ii d_i
      nh[i] = h.eh[i] / h.n;
      dot += nh[i] * ge[i];
      gsum += ge[i];
    }
    float geh[3], ehsum = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { geh[i] = (c / h.n) * (ge[i] - nh[i] * dot); ehsum += geh[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) geps[i] = geh[i] - ehsum / 3.f + gsum / 3.f;
    cl_eps_to_sigma(s, geps, gs);
    const M3 Y = cl_udv_adjoint(U, s, V, G, d, gs);
#pragma unroll
    for (int i = 0; i < 9; ++i) gF.m[i] = yield ? Y.m[i] : G.m[i];
    a0 = yield ? -c * dot : 0.f;                    // dc / d log_E = -c
    a1 = yield ? dot / (2.f * P.mu) : 0.f;          // dc / d sigma_y
    return gF;
  }
  float q;
  bool moved;
  const bool yield = cl_drucker_prager(h, P, d, q, moved);
  float dot = 0.f, gsum = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ge[i] = (UtG.m[3 * i] * V.m[i] + UtG.m[3 * i + 1] * V.m[3 + i] + UtG.m[3 * i + 2] * V.m[6 + i]) * d[i];
    nh[i] = h.eh[i] / h.n;
    dot += nh[i] * ge[i];
    gsum += ge[i];
  }
  // projected side (delta_gamma > 0): e_i = tr / 3 - q eh_i / n with q = k (tr - 3 cohesion) alpha, k = (3 la + 2 mu) / (2 mu)
  // (k does not depend on E, so d/d log_E = 0); inside the cone e = eps; expanding side e = cohesion
  const float alpha = cl_dp_alpha(P.p2);
  const float k = (3.f * P.la + 2.f * P.mu) / (2.f * P.mu);
  float geh[3], ehsum = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) { geh[i] = (-q / h.n) * (ge[i] - nh[i] * dot); ehsum += geh[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float proj = geh[i] - ehsum / 3.f + gsum / 3.f - dot * k * alpha;
    geps[i] = yield ? (moved ? proj : ge[i]) : 0.f;
  }
  cl_eps_to_sigma(s, geps, gs);
  const float sp = sinf(P.p2 * kDeg), cp = cosf(P.p2 * kDeg);
  const float dalpha = kSqrt23 * 6.f / ((3.f - sp) * (3.f - sp)) * cp * kDeg;
  const float sh = h.tr - P.p3 * 3.f;
  a1 = (yield && moved) ? -dot * k * sh * dalpha : 0.f;
  return cl_udv_adjoint(U, s, V, G, d, gs);
}

template <int LAW>
__global__ void __launch_bounds__(kClThreads) k_classical_fwd(int n, int mode, const float* __restrict__ sc,
                                                              const float* __restrict__ F, float* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const ClParams P = cl_params<LAW>(sc);
  m3_store(out + 9 * (size_t)p, cl_forward<LAW>(m3_load(F + 9 * (size_t)p), P, mode));
}

template <int LAW>
__global__ void __launch_bounds__(kClThreads) k_classical_bwd(int n, int mode, const float* __restrict__ sc,
                                                              const float* __restrict__ F, const float* __restrict__ G,
                                                              float* __restrict__ gF, double* __restrict__ part) {
  __shared__ double sh[8];
  const ClParams P = cl_params<LAW>(sc);
  double acc[2] = {0.0, 0.0};
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    float a0, a1;
    m3_store(gF + 9 * (size_t)p, cl_backward<LAW>(m3_load(F + 9 * (size_t)p), m3_load(G + 9 * (size_t)p), P, mode, a0, a1));
    acc[0] += (double)a0;
    acc[1] += (double)a1;
  }
  if (LAW == NM_LAW_SIGMA_PLASTIC) return;      // no learnable scalar
  const auto tot = nm_block_reduce<4, NmSum>(acc, sh);      // nm_reduce.h: the fixed order
  if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = tot[threadIdx.x];
}

// one block: the per-block partials, out[j] = sum
__global__ void __launch_bounds__(kClThreads) k_classical_reduce(int nb, const double* __restrict__ part, float* __restrict__ out) {
  __shared__ double sh[8];
  const auto tot = nm_block_sum_partials<4, 2>(part, nb, 2, sh);
  if (threadIdx.x < 2) out[threadIdx.x] = (float)tot[threadIdx.x];
}

int cl_blocks(int n) {
  const int nb = nm_div_up(n, kClThreads);
  return nb < kClMaxBlocks ? nb : kClMaxBlocks;
}

bool cl_law_ok(int law) { return law >= NM_LAW_COROTATED && law <= NM_LAW_DRUCKER_PRAGER; }
bool cl_law_has_scalars(int law) { return law != NM_LAW_IDENTITY && law != NM_LAW_SIGMA_PLASTIC; }

}  // namespace

#define CL_DISPATCH(law, WHAT)                        \
  switch (law) {                                      \
    case NM_LAW_COROTATED: WHAT(NM_LAW_COROTATED); break;           \
    case NM_LAW_STVK: WHAT(NM_LAW_STVK); break;                     \
    case NM_LAW_VOLUME: WHAT(NM_LAW_VOLUME); break;                 \
    case NM_LAW_SIGMA: WHAT(NM_LAW_SIGMA); break;                   \
    case NM_LAW_SIGMA_PLASTIC: WHAT(NM_LAW_SIGMA_PLASTIC); break;   \
    case NM_LAW_VON_MISES: WHAT(NM_LAW_VON_MISES); break;           \
    default: WHAT(NM_LAW_DRUCKER_PRAGER); break;                    \
  }

extern "C" int nm_classical_fwd(int32_t n, int32_t law, int32_t mode, const float* scalars, const float* F, float* out,
                                void* stream) {
  NM_REQUIRE(n >= 0, "negative n");
  NM_REQUIRE(cl_law_ok(law), "unknown law");
  NM_REQUIRE(law != NM_LAW_VOLUME || mode == NM_VOLUME_ZIRAN || mode == NM_VOLUME_TAICHI, "unknown mode of the volume law");
  NM_REQUIRE(!cl_law_has_scalars(law) || scalars, "null scalars");
  NM_REQUIRE(n == 0 || (F && out), "null pointer");
  if (n == 0) return NM_OK;
  hipStream_t s = (hipStream_t)stream;
  if (law == NM_LAW_IDENTITY) {
    if (out != F) NM_HIP_CHECK(hipMemcpyAsync(out, F, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return NM_OK;
  }
#define CL_FWD(L) NM_LAUNCH(k_classical_fwd<L>, dim3(nm_div_up(n, kClThreads)), dim3(kClThreads), 0, s, (int)n, (int)mode, scalars, F, out)
  CL_DISPATCH(law, CL_FWD)
#undef CL_FWD
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" size_t nm_classical_bwd_workspace(int32_t n) {
  return n <= 0 ? 0 : (size_t)cl_blocks(n) * 2 * sizeof(double);
}

extern "C" int nm_classical_bwd(int32_t n, int32_t law, int32_t mode, const float* scalars, const float* F, const float* grad_out,
                                float* grad_F, float* grad_scalars, void* workspace, size_t workspace_bytes, void* stream) {
  NM_REQUIRE(n >= 0, "negative n");
  NM_REQUIRE(cl_law_ok(law), "unknown law");
  NM_REQUIRE(law != NM_LAW_VOLUME || mode == NM_VOLUME_ZIRAN || mode == NM_VOLUME_TAICHI, "unknown mode of the volume law");
  const bool learn = cl_law_has_scalars(law);
  NM_REQUIRE(!learn || (scalars && grad_scalars), "null scalars");
  NM_REQUIRE(n == 0 || (F && grad_out && grad_F), "null pointer");
  NM_REQUIRE(n == 0 || !learn || workspace, "null workspace");
  NM_REQUIRE(n == 0 || !learn || workspace_bytes >= nm_classical_bwd_workspace(n), "workspace too small (nm_classical_bwd_workspace)");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (learn) NM_HIP_CHECK(hipMemsetAsync(grad_scalars, 0, 2 * sizeof(float), s));
    return NM_OK;
  }
  if (law == NM_LAW_IDENTITY) {
    if (grad_F != grad_out) NM_HIP_CHECK(hipMemcpyAsync(grad_F, grad_out, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return NM_OK;
  }
  const int nb = cl_blocks(n);
  double* part = (double*)workspace;
#define CL_BWD(L) NM_LAUNCH(k_classical_bwd<L>, dim3(nb), dim3(kClThreads), 0, s, (int)n, (int)mode, scalars, F, grad_out, grad_F, part)
  CL_DISPATCH(law, CL_BWD)
#undef CL_BWD
  NM_LAUNCH_CHECK();
  if (learn) {
    NM_LAUNCH(k_classical_reduce, dim3(1), dim3(kClThreads), 0, s, nb, (const double*)part, grad_scalars);
    NM_LAUNCH_CHECK();
  }
  return NM_OK;
}
