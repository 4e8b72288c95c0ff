// Gaussian registration (experiments/regist.py): the per-Gaussian transform + covariance build and its adjoint reduced to
// 17 scalars, and the SSIM loss with its adjoint.
//   nm_regist_apply     Register.forward (modules/tune/regist/register.py) + general_utils.py:93-139, one thread per Gaussian
//   nm_regist_backward  its adjoint; per-block fp64 partials, then one workgroup sums them (nm_reduce.h): no atomics
//   nm_ssim_loss        modules/d3gs/utils/loss_utils.py:26-66 fused with its adjoint (separable 11-tap passes over LDS tiles)
#include "nm_common.h"
#include "nm_gaussian.h"
#include "nm_reduce.h"
#include "nm_ssim.h"
#include "nm_workspace.h"

namespace {

// ---------------------------------------------------------------- transform

struct RegParams {
  float R[9], q[4], s, t[3], o[3];
};

__device__ __forceinline__ RegParams load_params(const float* __restrict__ p) {
  RegParams P;
#pragma unroll
  for (int i = 0; i < 9; ++i) P.R[i] = p[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) P.q[i] = p[9 + i];
  P.s = p[13];
#pragma unroll
  for (int i = 0; i < 3; ++i) { P.t[i] = p[14 + i]; P.o[i] = p[17 + i]; }
  return P;
}

// quaternion_multiply(q0, q1) of transform_utils.py:14-23 (wxyz)
__device__ __forceinline__ void qmul(const float* a, const float* b, float* m) {
  const float w0 = a[0], x0 = a[1], y0 = a[2], z0 = a[3];
  const float w1 = b[0], x1 = b[1], y1 = b[2], z1 = b[3];
  m[0] = -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0;
  m[1] = x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0;
  m[2] = -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0;
  m[3] = x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0;
}

// Everything the forward and the adjoint share for one Gaussian.
struct RegFwd {
  float d[3];       // s (xyz - o)
  float u[3];       // xyz - o
  float qi[4];      // normalize(rot)
  float qm[4];      // quaternion_multiply(qi, q_R)
  float lm;         // |qm| (clamped)
  float qn[4];      // normalize(qm)  (= the stored rotation)
  float ln;         // build_rotation's own norm of qn
  float qb[4];      // qn / ln
  float M[9];       // build_rotation(qn)
  float e[3];       // scale_modifier * exp(log_scales + log s)
  float sig[3];     // log_scales + log s
};

__device__ __forceinline__ void reg_forward(int i, const float* __restrict__ xyz, const float* __restrict__ ls,
                                            const float* __restrict__ rot, const RegParams& P, float mod, RegFwd& f) {
  const float logs = logf(P.s);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f.u[a] = xyz[3 * i + a] - P.o[a];
    f.d[a] = P.s * f.u[a];
    f.sig[a] = ls[3 * i + a] + logs;
    f.e[a] = mod * expf(f.sig[a]);
  }
  const float4 r4 = reinterpret_cast<const float4*>(rot)[i];
  const float rq[4] = {r4.x, r4.y, r4.z, r4.w};
  qnormalize(rq, f.qi);
  qmul(f.qi, P.q, f.qm);
  f.lm = qnormalize(f.qm, f.qn);
  f.ln = sqrtf(f.qn[0] * f.qn[0] + f.qn[1] * f.qn[1] + f.qn[2] * f.qn[2] + f.qn[3] * f.qn[3]);
#pragma unroll
  for (int a = 0; a < 4; ++a) f.qb[a] = f.qn[a] / f.ln;
  quat_rot(f.qb, f.M);
}

__global__ void __launch_bounds__(256) k_regist_apply(int K, const float* __restrict__ xyz, const float* __restrict__ ls,
                                                      const float* __restrict__ rot, const float* __restrict__ params, float mod,
                                                      float* __restrict__ means3D, float* __restrict__ cov6,
                                                      float* __restrict__ out_ls, float* __restrict__ out_rot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  const RegParams P = load_params(params);
  RegFwd f;
  reg_forward(i, xyz, ls, rot, P, mod, f);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    means3D[3 * i + a] = P.R[3 * a + 0] * f.d[0] + P.R[3 * a + 1] * f.d[1] + P.R[3 * a + 2] * f.d[2] + P.t[a];
  cov6_build(f.M, f.e, cov6, i);
  if (out_ls) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_ls[3 * i + a] = f.sig[a];
  }
  if (out_rot) reinterpret_cast<float4*>(out_rot)[i] = make_float4(f.qn[0], f.qn[1], f.qn[2], f.qn[3]);
}

constexpr int kRegThreads = 256;
constexpr int kRegMaxBlocks = 512;
constexpr int kRegN = 17;

static int regist_blocks(int K) {
  const int b = nm_div_up(K, kRegThreads);
  return b < 1 ? 1 : (b > kRegMaxBlocks ? kRegMaxBlocks : b);
}

__global__ void __launch_bounds__(kRegThreads) k_regist_bwd(int K, const float* __restrict__ xyz, const float* __restrict__ ls,
                                                            const float* __restrict__ rot, const float* __restrict__ params,
                                                            float mod, const float* __restrict__ gm, const float* __restrict__ gc,
                                                            double* __restrict__ part) {
  __shared__ double sh[4 * kRegN];
  const RegParams P = load_params(params);
  double acc[kRegN];
#pragma unroll
  for (int j = 0; j < kRegN; ++j) acc[j] = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
    RegFwd f;
    reg_forward(i, xyz, ls, rot, P, mod, f);
    const float dp[3] = {gm[3 * i], gm[3 * i + 1], gm[3 * i + 2]};
    // means3D = R d + t
    float dd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[3 * a + b] += (double)(dp[a] * f.d[b]);
      acc[14 + a] += (double)dp[a];
      dd[a] = P.R[a] * dp[0] + P.R[3 + a] * dp[1] + P.R[6 + a] * dp[2];
    }
    float ds = dd[0] * f.u[0] + dd[1] * f.u[1] + dd[2] * f.u[2];
    // cov6 = strip(L L^T)
    const float g6[6] = {gc[6 * i], gc[6 * i + 1], gc[6 * i + 2], gc[6 * i + 3], gc[6 * i + 4], gc[6 * i + 5]};
    float dM[9];
    cov6_adj(g6, f.M, f.e, dM, [&](int b, float de) { ds += de * f.e[b] / P.s; });      // e = mod exp(ls + log s): de/ds = e / s
    acc[13] += (double)ds;
    float dqb[4];
    quat_rot_adj(f.qb, dM, dqb);
    float dqn[4], dqm[4];
    norm_adj(f.qb, f.ln, dqb, dqn);      // build_rotation's own normalisation
    norm_adj(f.qn, f.lm, dqn, dqm);      // F.normalize of the product
    // quaternion_multiply(qi, q_R) w.r.t. q_R
    const float w0 = f.qi[0], x0 = f.qi[1], y0 = f.qi[2], z0 = f.qi[3];
    acc[9] += (double)(w0 * dqm[0] + x0 * dqm[1] + y0 * dqm[2] + z0 * dqm[3]);
    acc[10] += (double)(-x0 * dqm[0] + w0 * dqm[1] - z0 * dqm[2] + y0 * dqm[3]);
    acc[11] += (double)(-y0 * dqm[0] + z0 * dqm[1] + w0 * dqm[2] - x0 * dqm[3]);
    acc[12] += (double)(-z0 * dqm[0] - y0 * dqm[1] + x0 * dqm[2] + w0 * dqm[3]);
  }
  const auto tot = nm_block_reduce<4, NmSum>(acc, sh);
  if (threadIdx.x < kRegN) part[(size_t)blockIdx.x * kRegN + threadIdx.x] = tot[threadIdx.x];
}

// one block: the partials of every scalar, then out[j] += sum
__global__ void __launch_bounds__(256) k_regist_reduce(int nb, const double* __restrict__ part, float* __restrict__ out) {
  __shared__ double sh[4 * kRegN];
  const auto tot = nm_block_sum_partials<4, kRegN>(part, nb, kRegN, sh);
  if (threadIdx.x < kRegN) out[threadIdx.x] = (float)((double)out[threadIdx.x] + tot[threadIdx.x]);
}

// ---------------------------------------------------------------- SSIM

constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct SsimDims {
  int h, w, tx, ty, nblk;
};

static SsimDims ssim_dims(int h, int w) {
  SsimDims d;
  d.h = h; d.w = w;
  d.tx = nm_div_up(w, kTW);
  d.ty = nm_div_up(h, kTH);
  d.nblk = 3 * d.tx * d.ty;
  return d;
}

// workspace: [part: one double per k_ssim_fwd workgroup, padded][maps: 9 h w floats, not padded]
static size_t ssim_part_bytes(const SsimDims& d) { return nm_align256((size_t)d.nblk * sizeof(double)); }

// Pass 1: five blurred moments per pixel, the SSIM map, its per-block fp64 sum and (maps != NULL) the three coefficient maps
// a = dS/dmu1, b = dS/dE[x^2], c = dS/dE[xy].
__global__ void __launch_bounds__(256) k_ssim_fwd(SsimDims D, Window W, const float* __restrict__ img, const float* __restrict__ gt,
                                                  double* __restrict__ part, float* __restrict__ maps) {
  __shared__ float sx[kLH][kLW], sy[kLH][kLW];
  __shared__ float hm[5][kLH][kTW];
  __shared__ double red[4];
  const int bx = blockIdx.x, by = blockIdx.y, ch = blockIdx.z;
  const int x0 = bx * kTW - kR, y0 = by * kTH - kR;
  const size_t plane = (size_t)D.h * D.w;
  const float* X = img + ch * plane;
  const float* Y = gt + ch * plane;
  for (int e = threadIdx.x; e < kLH * kLW; e += blockDim.x) {
    const int ly = e / kLW, lx = e % kLW;
    const int gy = y0 + ly, gx = x0 + lx;
    const bool in = gy >= 0 && gy < D.h && gx >= 0 && gx < D.w;
    sx[ly][lx] = in ? X[(size_t)gy * D.w + gx] : 0.f;
    sy[ly][lx] = in ? Y[(size_t)gy * D.w + gx] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float a = sx[ly][lx + k], b = sy[ly][lx + k], wk = W.w[k];
      m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
    }
    hm[0][ly][lx] = m1; hm[1][ly][lx] = m2; hm[2][ly][lx] = e11; hm[3][ly][lx] = e22; hm[4][ly][lx] = e12;
  }
  __syncthreads();
  double ssum = 0.0;
  for (int e = threadIdx.x; e < kTH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    const int gy = by * kTH + ly, gx = bx * kTW + lx;
    if (gy >= D.h || gx >= D.w) continue;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float wk = W.w[k];
#pragma unroll
      for (int m = 0; m < 5; ++m) v[m] += wk * hm[m][ly + k][lx];
    }
    const float mu1 = v[0], mu2 = v[1];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = v[2] - mu1_sq, s2 = v[3] - mu2_sq, s12 = v[4] - mu12;
    const float A1 = 2.f * mu12 + kC1, A2 = 2.f * s12 + kC2;
    const float B1 = mu1_sq + mu2_sq + kC1, B2 = s1 + s2 + kC2;
    const float S = (A1 * A2) / (B1 * B2);
    ssum += (double)S;
    if (maps) {
      const size_t p = ch * plane + (size_t)gy * D.w + gx;
      maps[p] = S * (2.f * mu2 / A1 - 2.f * mu2 / A2 - 2.f * mu1 / B1 + 2.f * mu1 / B2);
      maps[3 * plane + p] = -S / B2;
      maps[6 * plane + p] = 2.f * S / A2;
    }
  }
  ssum = nm_block_reduce<4, NmSum>(ssum, red);
  if (threadIdx.x == 0) part[((size_t)ch * D.ty + by) * D.tx + bx] = ssum;
}

// sum of the pass-1 partials by one workgroup: *loss += weight (1 - mean S)
__device__ void ssim_finish(const SsimDims& D, const double* __restrict__ part, float weight, float* __restrict__ loss) {
  __shared__ double red[4];
  const double sum = nm_block_sum_partials<4, 1>(part, D.nblk, 1, red)[0];
  if (threadIdx.x == 0) {
    const double mean = sum / (3.0 * (double)D.h * (double)D.w);
    *loss = (float)((double)*loss + (double)weight * (1.0 - mean));
  }
}

// Pass 2: blur the three coefficient maps (the adjoint of a zero-padded symmetric correlation is the same correlation) and
// dL/dx_p += -weight / N (Ga + 2 x_p Gb + y_p Gc); workgroup (0,0,0) also finishes the loss.
__global__ void __launch_bounds__(256) k_ssim_bwd(SsimDims D, Window W, float weight, const float* __restrict__ img,
                                                  const float* __restrict__ gt, const double* __restrict__ part,
                                                  const float* __restrict__ maps, float* __restrict__ loss, float* __restrict__ grad) {
  __shared__ float sm[3][kLH][kLW];
  __shared__ float hm[3][kLH][kTW];
  const int bx = blockIdx.x, by = blockIdx.y, ch = blockIdx.z;
  if (bx == 0 && by == 0 && ch == 0) {
    ssim_finish(D, part, weight, loss);
    __syncthreads();
  }
  if (!grad) return;
  const int x0 = bx * kTW - kR, y0 = by * kTH - kR;
  const size_t plane = (size_t)D.h * D.w;
  for (int e = threadIdx.x; e < kLH * kLW; e += blockDim.x) {
    const int ly = e / kLW, lx = e % kLW;
    const int gy = y0 + ly, gx = x0 + lx;
    const bool in = gy >= 0 && gy < D.h && gx >= 0 && gx < D.w;
    const size_t p = ch * plane + (size_t)gy * D.w + gx;
#pragma unroll
    for (int m = 0; m < 3; ++m) sm[m][ly][lx] = in ? maps[m * 3 * plane + p] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float wk = W.w[k];
      v0 += wk * sm[0][ly][lx + k]; v1 += wk * sm[1][ly][lx + k]; v2 += wk * sm[2][ly][lx + k];
    }
    hm[0][ly][lx] = v0; hm[1][ly][lx] = v1; hm[2][ly][lx] = v2;
  }
  __syncthreads();
  const float scale = -weight / (3.f * (float)D.h * (float)D.w);
  for (int e = threadIdx.x; e < kTH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    const int gy = by * kTH + ly, gx = bx * kTW + lx;
    if (gy >= D.h || gx >= D.w) continue;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float wk = W.w[k];
      v0 += wk * hm[0][ly + k][lx]; v1 += wk * hm[1][ly + k][lx]; v2 += wk * hm[2][ly + k][lx];
    }
    const size_t p = ch * plane + (size_t)gy * D.w + gx;
    grad[p] += scale * (v0 + 2.f * img[p] * v1 + gt[p] * v2);
  }
}

}  // namespace

extern "C" int nm_regist_apply(int32_t k, const float* xyz, const float* log_scales, const float* rot, const float* params,
                               float scale_modifier, float* means3D, float* cov6, float* out_log_scales, float* out_rot,
                               void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(xyz && log_scales && rot && params && means3D && cov6, "null pointer");
  NM_REQUIRE(((uintptr_t)rot | (uintptr_t)out_rot) % 16 == 0, "rot / out_rot must be 16-byte aligned");
  NM_LAUNCH(k_regist_apply, dim3(nm_div_up(k, 256)), dim3(256), 0, (hipStream_t)stream, (int)k, xyz, log_scales, rot, params,
            scale_modifier, means3D, cov6, out_log_scales, out_rot);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" size_t nm_regist_bwd_workspace(int32_t k) {
  return (size_t)regist_blocks(k < 0 ? 0 : k) * kRegN * sizeof(double);
}

extern "C" int nm_regist_backward(int32_t k, const float* xyz, const float* log_scales, const float* rot, const float* params,
                                  float scale_modifier, const float* dL_dmeans3D, const float* dL_dcov6, float* dL_dparams,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  NM_REQUIRE(params && dL_dparams && workspace, "null pointer");
  NM_REQUIRE(k == 0 || (xyz && log_scales && rot && dL_dmeans3D && dL_dcov6), "null pointer");
  NM_REQUIRE(k == 0 || (uintptr_t)rot % 16 == 0, "rot must be 16-byte aligned");
  const int nb = regist_blocks(k);
  NM_REQUIRE(workspace_bytes >= (size_t)nb * kRegN * sizeof(double), "workspace too small (nm_regist_bwd_workspace)");
  double* part = (double*)workspace;
  NM_LAUNCH(k_regist_bwd, dim3(nb), dim3(kRegThreads), 0, (hipStream_t)stream, (int)k, xyz, log_scales, rot, params,
            scale_modifier, dL_dmeans3D, dL_dcov6, part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_regist_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, nb, (const double*)part, dL_dparams);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" size_t nm_ssim_workspace(int32_t h, int32_t w) {
  if (h <= 0 || w <= 0) return 0;
  return ssim_part_bytes(ssim_dims(h, w)) + (size_t)9 * h * w * sizeof(float);
}

extern "C" int nm_ssim_loss(float weight, int32_t h, int32_t w, const float* img, const float* gt, float* loss_out, float* dL_dimg,
                            void* workspace, size_t workspace_bytes, void* stream) {
  NM_REQUIRE(h > 0 && w > 0 && img && gt && loss_out && workspace, "bad arguments");
  const SsimDims D = ssim_dims(h, w);
  NM_REQUIRE(workspace_bytes >= nm_ssim_workspace(h, w), "workspace too small (nm_ssim_workspace)");
  double* part = (double*)workspace;
  float* maps = dL_dimg ? (float*)((char*)workspace + ssim_part_bytes(D)) : nullptr;
  const Window W = ssim_window();
  NM_LAUNCH(k_ssim_fwd, dim3(D.tx, D.ty, 3), dim3(256), 0, (hipStream_t)stream, D, W, img, gt, part, maps);
  NM_LAUNCH_CHECK();
  const dim3 g2 = dL_dimg ? dim3(D.tx, D.ty, 3) : dim3(1, 1, 1);
  NM_LAUNCH(k_ssim_bwd, g2, dim3(256), 0, (hipStream_t)stream, D, W, weight, img, gt, (const double*)part, (const float*)maps,
            loss_out, dL_dimg);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
