// Image-quality metrics of experiments/evaluation.py: torchmetrics' PeakSignalNoiseRatio (the sum of squared errors) and
// structural_similarity_index_measure (gaussian window 11 / sigma 1.5, k1 0.01, k2 0.03, data_range = the inputs' range) for a
// batch of B images, with no host synchronisation and no atomics (two calls give identical bits).
//   k_metrics_stats   pass 1: per image min / max of both inputs and the fp64 sum of squared errors, one partial per workgroup
//   k_metrics_range   one workgroup: fixed-order finish of pass 1 -> sse_out[b] and c1 / c2 per image (own or batch-wide range)
//   k_metrics_ssim    pass 2: the SSIM map over the (H-10) x (W-10) windows lying inside the image, one fp64 partial per workgroup
//   k_metrics_finish  one workgroup per image: fixed-order sum of its partials -> ssim_out[b]
// torchmetrics reflect-pads by 5, convolves without padding and crops 5 from each side of the map: what is left is exactly the
// windows inside the image, so no padded pixel ever reaches the result and this file pads nothing.
#include "nm_common.h"
#include "nm_ssim.h"

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
static size_t align256(size_t v) { return (v + 255) / 256 * 256; }
static size_t ws_stat_bytes(const MetricDims& d) { return align256((size_t)d.b * kStatN * d.g1 * sizeof(double)); }
static size_t ws_img_bytes(const MetricDims& d) { return align256((size_t)d.b * 6 * sizeof(double)); }
static size_t ws_ssim_bytes(const MetricDims& d) { return align256((size_t)d.b * d.c * d.ty * d.tx * sizeof(double)); }

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
  __shared__ double red[4][kStatN];
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
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pmin = fminf(pmin, __shfl_xor(pmin, o, 64)); pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
    tmin = fminf(tmin, __shfl_xor(tmin, o, 64)); tmax = fmaxf(tmax, __shfl_xor(tmax, o, 64));
    sse += __shfl_xor(sse, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = pmin; red[wave][1] = pmax; red[wave][2] = tmin; red[wave][3] = tmax; red[wave][4] = sse;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* q = part + (size_t)img * kStatN * D.g1 + blockIdx.x;
    q[0 * D.g1] = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
    q[1 * D.g1] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
    q[2 * D.g1] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    q[3 * D.g1] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
    q[4 * D.g1] = ((red[0][4] + red[1][4]) + red[2][4]) + red[3][4];
  }
}

// One workgroup of 256.  Wave w finishes images w, w + 4, ... (lanes over the g1 partials, then a fixed shuffle tree):
// sse_out[b] and the image's min / max.  Then c1 = (0.01 dr)^2, c2 = (0.03 dr)^2 per image, dr = max(pmax - pmin, tmax - tmin)
// over that image (per_image) or over the whole batch (torchmetrics on a batched call).
__global__ void __launch_bounds__(256) k_metrics_range(MetricDims D, int per_image, const double* __restrict__ part,
                                                       double* __restrict__ stat, double* __restrict__ sse_out) {
  __shared__ double red[4][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int img = wave; img < D.b; img += 4) {
    const double* q = part + (size_t)img * kStatN * D.g1;
    double pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY, sse = 0.0;
    for (int j = lane; j < D.g1; j += 64) {
      pmin = fmin(pmin, q[j]); pmax = fmax(pmax, q[D.g1 + j]);
      tmin = fmin(tmin, q[2 * D.g1 + j]); tmax = fmax(tmax, q[3 * D.g1 + j]);
      sse += q[4 * D.g1 + j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      pmin = fmin(pmin, __shfl_xor(pmin, o, 64)); pmax = fmax(pmax, __shfl_xor(pmax, o, 64));
      tmin = fmin(tmin, __shfl_xor(tmin, o, 64)); tmax = fmax(tmax, __shfl_xor(tmax, o, 64));
      sse += __shfl_xor(sse, o, 64);
    }
    if (lane == 0) {
      double* s = stat + (size_t)img * 6;
      s[0] = pmin; s[1] = pmax; s[2] = tmin; s[3] = tmax;
      if (sse_out) sse_out[img] = sse;
    }
  }
  __syncthreads();                 // (also orders the global writes above for the reads below: one workgroup)
  double bmin_p = INFINITY, bmax_p = -INFINITY, bmin_t = INFINITY, bmax_t = -INFINITY;
  if (!per_image) {
    for (int img = threadIdx.x; img < D.b; img += blockDim.x) {
      const double* s = stat + (size_t)img * 6;
      bmin_p = fmin(bmin_p, s[0]); bmax_p = fmax(bmax_p, s[1]); bmin_t = fmin(bmin_t, s[2]); bmax_t = fmax(bmax_t, s[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      bmin_p = fmin(bmin_p, __shfl_xor(bmin_p, o, 64)); bmax_p = fmax(bmax_p, __shfl_xor(bmax_p, o, 64));
      bmin_t = fmin(bmin_t, __shfl_xor(bmin_t, o, 64)); bmax_t = fmax(bmax_t, __shfl_xor(bmax_t, o, 64));
    }
    if (lane == 0) { red[wave][0] = bmin_p; red[wave][1] = bmax_p; red[wave][2] = bmin_t; red[wave][3] = bmax_t; }
    __syncthreads();
    bmin_p = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
    bmax_p = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
    bmin_t = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    bmax_t = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
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
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = red[0];
#pragma unroll
    for (int i = 1; i < kSsimWaves; ++i) acc += red[i];
    part[((size_t)plane_id * D.ty + by) * D.tx + bx] = acc;
  }
}

// grid (B): ssim_out[b] = (fixed-order sum of image b's C * ty * tx partials) / (C (H - 10) (W - 10))
__global__ void __launch_bounds__(256) k_metrics_finish(MetricDims D, const double* __restrict__ part, double* __restrict__ ssim_out) {
  __shared__ double red[4];
  const int img = blockIdx.x;
  const int np = D.c * D.ty * D.tx;
  const double* q = part + (size_t)img * np;
  double acc = 0.0;
  for (int j = threadIdx.x; j < np; j += blockDim.x) acc += q[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    ssim_out[img] = (((red[0] + red[1]) + red[2]) + red[3]) / ((double)D.c * (double)(D.h - 2 * kR) * (double)(D.w - 2 * kR));
}

}  // namespace

extern "C" size_t nm_image_metrics_workspace(int32_t b, int32_t c, int32_t h, int32_t w) {
  if (b <= 0 || c <= 0 || h < kWin || w < kWin) return 0;
  const MetricDims d = metric_dims(b, c, h, w);
  return ws_stat_bytes(d) + ws_img_bytes(d) + ws_ssim_bytes(d);
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
  double* part1 = (double*)workspace;
  double* stat = (double*)((char*)workspace + ws_stat_bytes(D));
  double* part2 = (double*)((char*)workspace + ws_stat_bytes(D) + ws_img_bytes(D));
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
