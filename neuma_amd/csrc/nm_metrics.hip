// Image-quality metrics of experiments/evaluation.py: torchmetrics' PeakSignalNoiseRatio (the sum of squared errors) and
// structural_similarity_index_measure (gaussian window 11 / sigma 1.5, k1 0.01, k2 0.03, data_range = the inputs' range) for a
// batch of B images, with no host synchronisation and no atomics: every reduction is nm_reduce.h's, so two calls give identical bits.
//   k_metrics_stats   pass 1: per image min / max of both inputs and the fp64 sum of squared errors, one partial per workgroup
//   k_metrics_range   one workgroup: finish of pass 1 -> sse_out[b] and c1 / c2 per image (own or batch-wide range)
//   k_metrics_ssim    pass 2: the SSIM map over the (H-10) x (W-10) windows lying inside the image, one fp64 partial per workgroup
//   k_metrics_finish  one workgroup per image: sum of its partials -> ssim_out[b]
// torchmetrics reflect-pads by 5, convolves without padding and crops 5 from each side of the map: what is left is exactly the
// windows inside the image, so no padded pixel ever reaches the result and this file pads nothing.
#include "nm_common.h"
#include "nm_reduce.h"
#include "nm_ssim.h"
#include "nm_workspace.h"

namespace {

// pass 2: one workgroup per CU (82 KB of LDS), so eight waves rather than four to cover its loads (4.40 -> 3.12 ms at 16 x 1080p)
constexpr int kSsimThreads = 512, kSsimWaves = kSsimThreads / 64;
constexpr int kStatThreads = 256;
constexpr int kStatMaxBlocks = 128;   // pass-1 workgroups per image
constexpr int kStatN = 5;             // pmin, pmax, tmin, tmax, sse

struct MetricDims {
  int b, c, h, w;
  int64_t n;         // c * h * w
  int g1;            // pass-1 workgroups per image
  int tx, ty;        // pass-2 tiles over the valid windows
};

static MetricDims metric_dims(int b, int c, int h, int w) {
  MetricDims d;
  d.b = b; d.c = c; d.h = h; d.w = w;
  d.n = (int64_t)c * h * w;
  const int g = nm_div_up(d.n, kStatThreads * 16);
  d.g1 = g < 1 ? 1 : (g > kStatMaxBlocks ? kStatMaxBlocks : g);
  d.tx = nm_div_up(w - 2 * kR, kTW);
  d.ty = nm_div_up(h - 2 * kR, kTH);
  return d;
}

// workspace: [stat partials B x 5 x g1][per image pmin, pmax, tmin, tmax, c1, c2: B x 6][ssim partials B x C x ty x tx], fp64
struct MetricWs { double *part1, *stat, *part2; size_t total; };
static MetricWs carve_metric_ws(void* base, const MetricDims& d) {
  NmCarver c(base);
  MetricWs w;
  w.part1 = c.take<double>((size_t)d.b * kStatN * d.g1);
  w.stat = c.take<double>((size_t)d.b * 6);
  w.part2 = c.take<double>((size_t)d.b * d.c * d.ty * d.tx);
  w.total = c.total();
  return w;
}

// pass 1's five accumulators {pmin, tmin, pmax, tmax, sse} in one reduction
struct StatOp {
  __device__ __forceinline__ static double apply(int j, double a, double b) { return j == 4 ? a + b : NmMinMax<2>::apply(j, a, b); }
};

__device__ __forceinline__ void stat_elem(float p, float t, float& pmin, float& pmax, float& tmin, float& tmax, double& sse) {
  pmin = fminf(pmin, p); pmax = fmaxf(pmax, p);
  tmin = fminf(tmin, t); tmax = fmaxf(tmax, t);
  const double d = (double)p - (double)t;      // exact in fp64
  sse += d * d;
}

// Pass 1.  grid (g1, B): workgroup x of image y strides over the image's n values (float4 when V == 4) in a fixed order.
template <int V>
__global__ void __launch_bounds__(kStatThreads) k_metrics_stats(MetricDims D, const float* __restrict__ preds,
                                                               const float* __restrict__ target, double* __restrict__ part) {
  __shared__ double red[4 * kStatN];
  const int img = blockIdx.y;
  const float* P = preds + (size_t)img * D.n;
  const float* T = target + (size_t)img * D.n;
  float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
  double sse = 0.0;
  const int64_t stride = (int64_t)D.g1 * kStatThreads;
  if (V == 4) {
    const int64_t n4 = D.n / 4;
    const float4* P4 = reinterpret_cast<const float4*>(P);
    const float4* T4 = reinterpret_cast<const float4*>(T);
    for (int64_t i = (int64_t)blockIdx.x * kStatThreads + threadIdx.x; i < n4; i += stride) {
      const float4 p = P4[i], t = T4[i];
      stat_elem(p.x, t.x, pmin, pmax, tmin, tmax, sse);
      stat_elem(p.y, t.y, pmin, pmax, tmin, tmax, sse);
      stat_elem(p.z, t.z, pmin, pmax, tmin, tmax, sse);
      stat_elem(p.w, t.w, pmin, pmax, tmin, tmax, sse);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kStatThreads + threadIdx.x; i < D.n; i += stride)
      stat_elem(P[i], T[i], pmin, pmax, tmin, tmax, sse);
  }
  const double st[kStatN] = {(double)pmin, (double)tmin, (double)pmax, (double)tmax, sse};      // (the partials are fp64)
  const auto tot = nm_block_reduce<4, StatOp>(st, red);
  if (threadIdx.x == 0) {
    double* q = part + (size_t)img * kStatN * D.g1 + blockIdx.x;
    q[0 * D.g1] = tot[0];
    q[1 * D.g1] = tot[2];
    q[2 * D.g1] = tot[1];
    q[3 * D.g1] = tot[3];
    q[4 * D.g1] = tot[4];
  }
}

// One workgroup of 256.  Wave w finishes images w, w + 4, ... (lanes over the g1 partials, then the wave reduce):
// sse_out[b] and the image's min / max.  Then c1 = (0.01 dr)^2, c2 = (0.03 dr)^2 per image, dr = max(pmax - pmin, tmax - tmin)
// over that image (per_image) or over the whole batch (torchmetrics on a batched call).
__global__ void __launch_bounds__(256) k_metrics_range(MetricDims D, int per_image, const double* __restrict__ part,
                                                       double* __restrict__ stat, double* __restrict__ sse_out) {
  __shared__ double red[4 * 4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int img = wave; img < D.b; img += 4) {
    const double* q = part + (size_t)img * kStatN * D.g1;
    double pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY, sse = 0.0;
    for (int j = lane; j < D.g1; j += 64) {
      pmin = fmin(pmin, q[j]); pmax = fmax(pmax, q[D.g1 + j]);
      tmin = fmin(tmin, q[2 * D.g1 + j]); tmax = fmax(tmax, q[3 * D.g1 + j]);
      sse += q[4 * D.g1 + j];
    }
    pmin = nm_wave_reduce<NmMin>(pmin); pmax = nm_wave_reduce<NmMax>(pmax);
    tmin = nm_wave_reduce<NmMin>(tmin); tmax = nm_wave_reduce<NmMax>(tmax);
    sse = nm_wave_reduce<NmSum>(sse);
    if (lane == 0) {
      double* s = stat + (size_t)img * 6;
      s[0] = pmin; s[1] = pmax; s[2] = tmin; s[3] = tmax;
      if (sse_out) sse_out[img] = sse;
    }
  }
  __syncthreads();                 // (also orders the global writes above for the reads below: one workgroup)
  double bmin_p = INFINITY, bmax_p = -INFINITY, bmin_t = INFINITY, bmax_t = -INFINITY;
  if (!per_image) {
    double r[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};      // pmin, tmin, pmax, tmax
    for (int img = threadIdx.x; img < D.b; img += blockDim.x) {
      const double* s = stat + (size_t)img * 6;
      r[0] = fmin(r[0], s[0]); r[2] = fmax(r[2], s[1]); r[1] = fmin(r[1], s[2]); r[3] = fmax(r[3], s[3]);
    }
    const auto tot = nm_block_reduce<4, NmMinMax<2>>(r, red);
    bmin_p = tot[0]; bmin_t = tot[1]; bmax_p = tot[2]; bmax_t = tot[3];
  }
  for (int img = threadIdx.x; img < D.b; img += blockDim.x) {
    double* s = stat + (size_t)img * 6;
    const double dr = per_image ? fmax(s[1] - s[0], s[3] - s[2]) : fmax(bmax_p - bmin_p, bmax_t - bmin_t);
    s[4] = (0.01 * dr) * (0.01 * dr);
    s[5] = (0.03 * dr) * (0.03 * dr);
  }
}

// Pass 2.  grid (tx, ty, B * C), 512 threads: a 16 x 64 tile of window origins, i.e. image pixels [oy, oy + 26) x [ox, ox + 74) -
// never below the image, and past its far edges only for windows that are not computed.  Moments in fp64 (the variances are differences of
// near-equal moments, and C2 is only 9e-4 of dr^2); the 26 x 74 input stays fp32 in LDS (x^2 and x y are exact in fp64).
__global__ void __launch_bounds__(kSsimThreads) k_metrics_ssim(MetricDims D, Window64 W, const float* __restrict__ preds,
                                                               const float* __restrict__ target, const double* __restrict__ stat,
                                                               double* __restrict__ part) {
  __shared__ float sx[kLH][kLW], sy[kLH][kLW];
  __shared__ double hm[5][kLH][kTW];
  __shared__ double red[kSsimWaves];
  const int bx = blockIdx.x, by = blockIdx.y, plane_id = blockIdx.z;      // plane_id = img * C + channel
  const int img = plane_id / D.c;
  const int ox = bx * kTW, oy = by * kTH;
  const size_t plane = (size_t)D.h * D.w;
  const float* X = preds + (size_t)plane_id * plane;
  const float* Y = target + (size_t)plane_id * plane;
  for (int e = threadIdx.x; e < kLH * kLW; e += blockDim.x) {
    const int ly = e / kLW, lx = e % kLW;
    const int gy = oy + ly, gx = ox + lx;
    const bool in = gy < D.h && gx < D.w;
    sx[ly][lx] = in ? X[(size_t)gy * D.w + gx] : 0.f;
    sy[ly][lx] = in ? Y[(size_t)gy * D.w + gx] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double a = sx[ly][lx + k], b = sy[ly][lx + k], wk = W.w[k];
      m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
    }
    hm[0][ly][lx] = m1; hm[1][ly][lx] = m2; hm[2][ly][lx] = e11; hm[3][ly][lx] = e22; hm[4][ly][lx] = e12;
  }
  __syncthreads();
  const double c1 = stat[(size_t)img * 6 + 4], c2 = stat[(size_t)img * 6 + 5];
  const int vh = D.h - 2 * kR, vw = D.w - 2 * kR;
  double ssum = 0.0;
  for (int e = threadIdx.x; e < kTH * kTW; e += blockDim.x) {
    const int ly = e / kTW, lx = e % kTW;
    if (oy + ly >= vh || ox + lx >= vw) continue;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double wk = W.w[k];
#pragma unroll
      for (int m = 0; m < 5; ++m) v[m] += wk * hm[m][ly + k][lx];
    }
    // torchmetrics 1.x _ssim_update: the two variances clamped at 0, the covariance not
    const double mu1 = v[0], mu2 = v[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = fmax(v[2] - mu1_sq, 0.0), s2 = fmax(v[3] - mu2_sq, 0.0), s12 = v[4] - mu12;
    const double upper = 2.0 * s12 + c2, lower = (s1 + s2) + c2;
    ssum += ((2.0 * mu12 + c1) * upper) / (((mu1_sq + mu2_sq) + c1) * lower);
  }
  ssum = nm_block_reduce<kSsimWaves, NmSum>(ssum, red);
  if (threadIdx.x == 0) part[((size_t)plane_id * D.ty + by) * D.tx + bx] = ssum;
}

// grid (B): ssim_out[b] = (sum of image b's C * ty * tx partials) / (C (H - 10) (W - 10))
__global__ void __launch_bounds__(256) k_metrics_finish(MetricDims D, const double* __restrict__ part, double* __restrict__ ssim_out) {
  __shared__ double red[4];
  const int img = blockIdx.x;
  const int np = D.c * D.ty * D.tx;
  const double sum = nm_block_sum_partials<4, 1>(part + (size_t)img * np, np, 1, red)[0];
  if (threadIdx.x == 0) ssim_out[img] = sum / ((double)D.c * (double)(D.h - 2 * kR) * (double)(D.w - 2 * kR));
}

}  // namespace

extern "C" size_t nm_image_metrics_workspace(int32_t b, int32_t c, int32_t h, int32_t w) {
  if (b <= 0 || c <= 0 || h < kWin || w < kWin) return 0;
  return carve_metric_ws(nullptr, metric_dims(b, c, h, w)).total;
}

extern "C" int nm_image_metrics(int32_t b, int32_t c, int32_t h, int32_t w, const float* preds, const float* target,
                                int32_t range_per_image, double* sse_out, double* ssim_out, void* workspace, size_t workspace_bytes,
                                void* stream) {
  NM_REQUIRE(b > 0 && c > 0, "b and c must be positive");
  NM_REQUIRE(h >= kWin && w >= kWin, "h and w must be at least 11 (the SSIM window)");
  NM_REQUIRE((int64_t)b * c <= 65535, "b * c above 65535");
  NM_REQUIRE(preds && target && sse_out && workspace, "null pointer");
  const MetricDims D = metric_dims(b, c, h, w);
  NM_REQUIRE(workspace_bytes >= nm_image_metrics_workspace(b, c, h, w), "workspace too small (nm_image_metrics_workspace)");
  const MetricWs ws = carve_metric_ws(workspace, D);
  double *part1 = ws.part1, *stat = ws.stat, *part2 = ws.part2;
  const hipStream_t s = (hipStream_t)stream;
  const bool vec4 = D.n % 4 == 0 && ((uintptr_t)preds | (uintptr_t)target) % 16 == 0;
  if (vec4)
    NM_LAUNCH(k_metrics_stats<4>, dim3(D.g1, b), dim3(kStatThreads), 0, s, D, preds, target, part1);
  else
    NM_LAUNCH(k_metrics_stats<1>, dim3(D.g1, b), dim3(kStatThreads), 0, s, D, preds, target, part1);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_metrics_range, dim3(1), dim3(256), 0, s, D, (int)(range_per_image != 0), (const double*)part1, stat, sse_out);
  NM_LAUNCH_CHECK();
  if (!ssim_out) return NM_OK;
  NM_LAUNCH(k_metrics_ssim, dim3(D.tx, D.ty, b * c), dim3(kSsimThreads), 0, s, D, ssim_window64(), preds, target, (const double*)stat, part2);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_metrics_finish, dim3(b), dim3(256), 0, s, D, (const double*)part2, ssim_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
