// LPIPS (VGG-16 trunk, five linear heads) as experiments/evaluation.py calls it: torchmetrics'
// LearnedPerceptualImagePatchSimilarity(net_type='vgg', normalize=True), one value per image pair.  Written from knowledge of
// torchmetrics / lpips; neither they nor torchvision were available to run against, so the yardstick is the fp64 restatement of
// the same definition in neuma_amd/extras/lpips.py.  For a, b (B, 3, H, W) in [0, 1], H, W >= 16:
//   x = (2 x - 1 - shift) / scale per channel; 13 convolutions 3x3 / pad 1 / bias / ReLU with 2x2 max-pools (floor) after
//   convolutions 2, 4, 7, 10; taps after the ReLU of 2, 4, 7, 10, 13; per tap and pixel t^ = t / sqrt(1e-8 + sum_c t^2),
//   d = sum_c w_c (a^_c - b^_c)^2; the value is the sum over the taps of the pixel mean of d.
// Activations are channels-last (N, H, W, C) fp32, so that the K index of the implicit GEMM is contiguous.
//   k_lpips_scale     (B,3,H,W) pair in [0,1] -> (2B,H,W,3) scaled, a's images first
//   k_conv3x3_c3      Cin = 3: plain VALU, one fmaf chain of 27 per output
//   k_conv3x3_mfma    Cin % 16 == 0: implicit GEMM on v_mfma_f32_16x16x4_f32, M = 64 output channels, N = 8 x 16 pixels,
//                     K = 9 * Cin in chunks of 16 channels; halo tile and weight slice in LDS; bias + ReLU in the epilogue
//   k_maxpool2        2x2 / stride 2 / floor
//   k_lpips_head      per pixel norms and weighted squared difference in fp64, one fp64 partial per workgroup
//   k_lpips_finish    one workgroup per pair: its partials in nm_reduce.h's order -> mean, set or added to out[pair]
// No atomics anywhere.  An output element of a convolution is ONE fmaf chain over k = (chunk, tap, channel) starting from 0
// (the f32 MFMA is bitwise that chain; zero padding enters as products with 0), then + bias: its bits depend on Cin alone, not on
// the image's slot in the batch, the pixel's place in its tile or the image size.  Two calls give identical bits.
#include "nm_common.h"
#include "nm_reduce.h"
#include "nm_workspace.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define NM_MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int kConvThreads = 256;
constexpr int kTM = 64;                     // output channels per workgroup (4 MFMA row tiles)
constexpr int kTH = 8, kTW = 16;            // pixel tile: each of the 4 waves owns 2 rows of 16 pixels
constexpr int kKC = 16;                     // input channels per K chunk
constexpr int kHaloH = kTH + 2, kHaloW = kTW + 2;
// LDS strides in floats, padded by 4: the 16 lanes of one ds_read_b128 phase then start on 16 different multiples of 4 banks
// (20 j mod 64 is a permutation of the multiples of 4 for j = 0..15; 148 = 2 * 64 + 20)
constexpr int kXS = kKC + 4;                // per halo pixel
constexpr int kWS = 9 * kKC + 4;            // per output channel
constexpr int kHaloVec = kHaloH * kHaloW * (kKC / 4);       // 720 float4 per chunk
constexpr int kHaloPer = (kHaloVec + kConvThreads - 1) / kConvThreads;      // 3
constexpr int kWVec = kTM * 9 * kKC / 4;                    // 2304 float4 per chunk
constexpr int kWPer = kWVec / kConvThreads;                 // 9
static_assert(kWVec % kConvThreads == 0, "weight slice must divide among the threads");

constexpr int kC3Threads = 256, kC3Pix = 64, kC3Co = 64;    // Cin = 3 kernel: 64 pixels x 4 groups of 16 output channels
constexpr int kHeadThreads = 256, kHeadWaves = 4, kHeadMaxBlocks = 256;

__constant__ float c_shift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float c_scale[3] = {0.458f, 0.448f, 0.450f};

// grid (blocks over H*W, 2B): image z < B from a, the others from b.
__global__ void __launch_bounds__(256) k_lpips_scale(int b, int h, int w, const float* __restrict__ a, const float* __restrict__ bb,
                                                     float* __restrict__ y) {
  const int img = blockIdx.y;
  const size_t plane = (size_t)h * w;
  const float* src = (img < b ? a + (size_t)img * 3 * plane : bb + (size_t)(img - b) * 3 * plane);
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= plane) return;
  float* q = y + ((size_t)img * plane + p) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = (2.f * src[c * plane + p] - 1.f - c_shift[c]) / c_scale[c];
}

// Cin = 3.  grid (blocks of 64 pixels, Cout / 64, N).  weight: (Cout, 27), k = tap * 3 + channel.
__global__ void __launch_bounds__(kC3Threads) k_conv3x3_c3(int cout, int h, int w, const float* __restrict__ x,
                                                           const float* __restrict__ weight, const float* __restrict__ bias,
                                                           float* __restrict__ y) {
  __shared__ float sw[kC3Co * 27];
  __shared__ float sb[kC3Co];
  const int m0 = blockIdx.y * kC3Co, img = blockIdx.z;
  for (int e = threadIdx.x; e < kC3Co * 27; e += kC3Threads) sw[e] = weight[(size_t)m0 * 27 + e];
  if (threadIdx.x < kC3Co) sb[threadIdx.x] = bias[m0 + threadIdx.x];
  __syncthreads();
  const int plane = h * w;
  const int p = blockIdx.x * kC3Pix + (threadIdx.x >> 2), cg = threadIdx.x & 3;
  if (p >= plane) return;
  const int oy = p / w, ox = p % w;
  const float* X = x + (size_t)img * plane * 3;
  float v[27];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int gy = oy + t / 3 - 1, gx = ox + t % 3 - 1;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[t * 3 + c] = in ? X[((size_t)gy * w + gx) * 3 + c] : 0.f;
  }
  float* Y = y + ((size_t)img * plane + p) * cout + m0 + cg * 16;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cg * 16 + q * 4 + r;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 27; ++k) acc = fmaf(sw[co * 27 + k], v[k], acc);
      o[r] = fmaxf(acc + sb[co], 0.f);
    }
    *reinterpret_cast<float4*>(Y + q * 4) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// Cin % 16 == 0, Cout % 64 == 0.  grid (tiles_x * tiles_y, Cout / 64, N), 256 threads.
// weight: (Cin / 16, Cout, 9, 16): for one chunk and 64 output channels a contiguous 64 x 144 slice, k = tap * 16 + channel.
// MFMA operands (16x16x4: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D row = 4 (l >> 4) + reg, col = l & 15): lane
// (i, g) reads the four consecutive channels 4 g .. 4 g + 3 of its output channel (A) or pixel (B) in one ds_read_b128 and feeds
// element s to step s, so step s multiplies channels {s, 4 + s, 8 + s, 12 + s}: a permutation of k both operands share.
__global__ void __launch_bounds__(kConvThreads) k_conv3x3_mfma(int cin, int cout, int h, int w, int tiles_x,
                                                               const float* __restrict__ x, const float* __restrict__ weight,
                                                               const float* __restrict__ bias, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float sW[kTM * kWS];
  __shared__ __attribute__((aligned(16))) float sX[kHaloH * kHaloW * kXS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int tx0 = (blockIdx.x % tiles_x) * kTW, ty0 = (blockIdx.x / tiles_x) * kTH;
  const int m0 = blockIdx.y * kTM, img = blockIdx.z;
  const float* X = x + (size_t)img * h * w * cin;

  // this thread's share of the halo: the same pixels for every chunk
  size_t xoff[kHaloPer];
  int xdst[kHaloPer];         // LDS float index, -1: none
  bool xin[kHaloPer];
#pragma unroll
  for (int r = 0; r < kHaloPer; ++r) {
    const int e = tid + r * kConvThreads;
    const int pix = e >> 2, q = e & 3;
    const int gy = ty0 + pix / kHaloW - 1, gx = tx0 + pix % kHaloW - 1;
    xdst[r] = e < kHaloVec ? pix * kXS + q * 4 : -1;
    xin[r] = e < kHaloVec && gy >= 0 && gy < h && gx >= 0 && gx < w;
    xoff[r] = xin[r] ? ((size_t)gy * w + gx) * cin + q * 4 : 0;
  }
  int wdst[kWPer];
#pragma unroll
  for (int r = 0; r < kWPer; ++r) {
    const int f = tid + r * kConvThreads;
    wdst[r] = (f / 36) * kWS + (f % 36) * 4;
  }

  // the next chunk's halo share and weight share wait in registers while the current chunk is multiplied
  f32x4 rx[kHaloPer], rw[kWPer];
#define NM_CONV_FETCH(chunk_)                                                                                             \
  do {                                                                                                                    \
    const float* Xc = X + (chunk_) * kKC;                                                                                 \
    const f32x4* Wc = reinterpret_cast<const f32x4*>(weight + ((size_t)(chunk_) * cout + m0) * (9 * kKC));               \
    _Pragma("unroll") for (int r = 0; r < kHaloPer; ++r)                                                                  \
      rx[r] = xin[r] ? *reinterpret_cast<const f32x4*>(Xc + xoff[r]) : f32x4{0.f, 0.f, 0.f, 0.f};                         \
    _Pragma("unroll") for (int r = 0; r < kWPer; ++r) rw[r] = Wc[tid + r * kConvThreads];                                 \
  } while (0)

  f32x4 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunk = cin / kKC;
  NM_CONV_FETCH(0);
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    __syncthreads();            // the previous chunk's readers are done
#pragma unroll
    for (int r = 0; r < kHaloPer; ++r)
      if (xdst[r] >= 0) *reinterpret_cast<f32x4*>(&sX[xdst[r]]) = rx[r];
#pragma unroll
    for (int r = 0; r < kWPer; ++r) *reinterpret_cast<f32x4*>(&sW[wdst[r]]) = rw[r];
    __syncthreads();
    // in flight under this chunk's MFMAs (the last chunk fetches itself again: one redundant fetch, no branch around 12 loads)
    NM_CONV_FETCH(chunk + 1 < nchunk ? chunk + 1 : chunk);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap % 3;
      float4 av[4], bv[2];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) av[mt] = *reinterpret_cast<const float4*>(&sW[(mt * 16 + li) * kWS + tap * kKC + lg * 4]);
#pragma unroll
      for (int t = 0; t < 2; ++t)
        bv[t] = *reinterpret_cast<const float4*>(&sX[((wave * 2 + t + dy) * kHaloW + li + dx) * kXS + lg * 4]);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          acc[mt][t] = NM_MFMA4(av[mt].x, bv[t].x, acc[mt][t]);
          acc[mt][t] = NM_MFMA4(av[mt].y, bv[t].y, acc[mt][t]);
          acc[mt][t] = NM_MFMA4(av[mt].z, bv[t].z, acc[mt][t]);
          acc[mt][t] = NM_MFMA4(av[mt].w, bv[t].w, acc[mt][t]);
        }
    }
  }

#undef NM_CONV_FETCH

  // epilogue: lane (i, g) holds output channels m0 + 16 mt + 4 g + {0..3} of pixel (row 2 wave + t, column i)
  const int ox = tx0 + li;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int oy = ty0 + wave * 2 + t;
    if (oy >= h || ox >= w) continue;
    float* Y = y + (((size_t)img * h + oy) * w + ox) * cout + m0 + lg * 4;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const float4 bq = *reinterpret_cast<const float4*>(bias + m0 + mt * 16 + lg * 4);
      const f32x4 v = acc[mt][t];
      *reinterpret_cast<float4*>(Y + mt * 16) =
          make_float4(fmaxf(v[0] + bq.x, 0.f), fmaxf(v[1] + bq.y, 0.f), fmaxf(v[2] + bq.z, 0.f), fmaxf(v[3] + bq.w, 0.f));
    }
  }
}

__device__ __forceinline__ float pool_max(float a, float b) { return b > a ? b : a; }

// (N, H, W, C) -> (N, H/2, W/2, C), C % 4 == 0.  One thread per output pixel and 4 channels.
__global__ void __launch_bounds__(256) k_maxpool2(size_t total, int c4, int h, int w, const float4* __restrict__ x,
                                                  float4* __restrict__ y) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int oh = h / 2, ow = w / 2;
  const int q = (int)(e % c4);
  size_t p = e / c4;
  const int ox = (int)(p % ow); p /= ow;
  const int oy = (int)(p % oh);
  const size_t img = p / oh;
  const float4* s = x + ((img * h + 2 * oy) * w + 2 * ox) * c4 + q;
  const float4 a = s[0], b = s[c4], c = s[(size_t)w * c4], d = s[(size_t)w * c4 + c4];
  y[e] = make_float4(pool_max(pool_max(a.x, b.x), pool_max(c.x, d.x)), pool_max(pool_max(a.y, b.y), pool_max(c.y, d.y)),
                     pool_max(pool_max(a.z, b.z), pool_max(c.z, d.z)), pool_max(pool_max(a.w, b.w), pool_max(c.w, d.w)));
}

static int head_blocks(int h, int w) {
  const int g = nm_div_up((int64_t)h * w, kHeadWaves * 8);
  return g < 1 ? 1 : (g > kHeadMaxBlocks ? kHeadMaxBlocks : g);
}

// grid (g, pairs): wave v of workgroup x takes pixels x * 4 + v, + 4 g, ... of its pair, one after the other; the lanes split the
// channels (4 consecutive each), everything after the loads in fp64.
__global__ void __launch_bounds__(kHeadThreads) k_lpips_head(int c, int plane, const float* __restrict__ ta,
                                                             const float* __restrict__ tb, const float* __restrict__ hw,
                                                             double* __restrict__ part) {
#pragma clang fp contract(off)      // u ia - v ib as fma(u, ia, -(v ib)) would round the two sides differently: d(a, b) != d(b, a)
  __shared__ double red[kHeadWaves];
  const int pair = blockIdx.y, g = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* A = ta + (size_t)pair * plane * c;
  const float* B = tb + (size_t)pair * plane * c;
  double dsum = 0.0;
  for (int p = blockIdx.x * kHeadWaves + wave; p < plane; p += g * kHeadWaves) {
    const float* pa = A + (size_t)p * c;
    const float* pb = B + (size_t)p * c;
    double na = 0.0, nb = 0.0;
    for (int k = lane * 4; k < c; k += 256) {
      const float4 u = *reinterpret_cast<const float4*>(pa + k), v = *reinterpret_cast<const float4*>(pb + k);
      na += (double)u.x * u.x + (double)u.y * u.y + (double)u.z * u.z + (double)u.w * u.w;
      nb += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    na = nm_wave_reduce<NmSum>(na);
    nb = nm_wave_reduce<NmSum>(nb);
    const double ia = 1.0 / sqrt(1e-8 + na), ib = 1.0 / sqrt(1e-8 + nb);
    double d = 0.0;
    for (int k = lane * 4; k < c; k += 256) {
      const float4 u = *reinterpret_cast<const float4*>(pa + k), v = *reinterpret_cast<const float4*>(pb + k);
      const float4 wq = *reinterpret_cast<const float4*>(hw + k);
      const double e0 = u.x * ia - v.x * ib, e1 = u.y * ia - v.y * ib, e2 = u.z * ia - v.z * ib, e3 = u.w * ia - v.w * ib;
      d += (double)wq.x * (e0 * e0) + (double)wq.y * (e1 * e1) + (double)wq.z * (e2 * e2) + (double)wq.w * (e3 * e3);
    }
    dsum += nm_wave_reduce<NmSum>(d);       // (the same value in every lane)
  }
  // every lane of a wave carries the wave's sum: the wave step of the block reduce would count it 64 times
  const double mine = lane == 0 ? dsum : 0.0;
  const double tot = nm_block_reduce<kHeadWaves, NmSum>(mine, red);
  if (threadIdx.x == 0) part[(size_t)pair * g + blockIdx.x] = tot;
}

// grid (pairs): out[pair] (+)= (sum of the pair's g partials) / plane
__global__ void __launch_bounds__(256) k_lpips_finish(int g, int plane, int accumulate, const double* __restrict__ part,
                                                      double* __restrict__ out) {
  __shared__ double red[4];
  const int pair = blockIdx.x;
  const double sum = nm_block_sum_partials<4, 1>(part + (size_t)pair * g, g, 1, red)[0];
  if (threadIdx.x == 0) {
    const double m = sum / (double)plane;
    out[pair] = accumulate ? out[pair] + m : m;
  }
}

// ---------------------------------------------------------------- host
static int conv_launch(int n, int cin, int cout, int h, int w, const float* x, const float* weight, const float* bias, float* y,
                       hipStream_t s) {
  if (cin == 3) {
    NM_LAUNCH(k_conv3x3_c3, dim3(nm_div_up((int64_t)h * w, kC3Pix), cout / kC3Co, n), dim3(kC3Threads), 0, s, cout, h, w, x, weight,
              bias, y);
  } else {
    const int tiles_x = nm_div_up(w, kTW), tiles_y = nm_div_up(h, kTH);
    NM_LAUNCH(k_conv3x3_mfma, dim3(tiles_x * tiles_y, cout / kTM, n), dim3(kConvThreads), 0, s, cin, cout, h, w, tiles_x, x,
              weight, bias, y);
  }
  NM_LAUNCH_CHECK();
  return NM_OK;
}

static int pool_launch(int n, int c, int h, int w, const float* x, float* y, hipStream_t s) {
  const size_t total = (size_t)n * (h / 2) * (w / 2) * (c / 4);
  if (total == 0) return NM_OK;
  NM_LAUNCH(k_maxpool2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, c / 4, h, w, (const float4*)x, (float4*)y);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

static int head_launch(int pairs, int c, int h, int w, const float* ta, const float* tb, const float* hw, double* out,
                       double* part, int accumulate, hipStream_t s) {
  const int g = head_blocks(h, w);
  NM_LAUNCH(k_lpips_head, dim3(g, pairs), dim3(kHeadThreads), 0, s, c, h * w, ta, tb, hw, part);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_lpips_finish, dim3(pairs), dim3(256), 0, s, g, h * w, accumulate, (const double*)part, out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

constexpr int kConvs = 13, kTaps = 5;
const int kCin[kConvs] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kCout[kConvs] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kTapAfter[kConvs] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};      // head index after this convolution's ReLU
const int kPoolAfter[kConvs] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0};

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// workspace: [scaled input 2B x H x W x 3][activations 2B x H x W x 64, twice][head partials B x kHeadMaxBlocks, fp64]
struct LpipsWs { float *scaled, *act[2]; double* part; size_t total; };
static LpipsWs carve_lpips_ws(void* base, int b, int h, int w) {
  NmCarver c(base);
  LpipsWs ws;
  const size_t px = (size_t)2 * b * h * w;
  ws.scaled = c.take<float>(px * 3);
  ws.act[0] = c.take<float>(px * 64);
  ws.act[1] = c.take<float>(px * 64);
  ws.part = c.take<double>((size_t)b * kHeadMaxBlocks);
  ws.total = c.total();
  return ws;
}

}  // namespace

extern "C" int nm_conv3x3_relu(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, const float* x, const float* weight,
                               const float* bias, float* y, void* stream) {
  NM_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0, "conv3x3: n in 1..65535, h and w positive");
  NM_REQUIRE((int64_t)h * w < (1 << 30), "conv3x3: h * w above 2^30");
  NM_REQUIRE(cin == 3 || (cin > 0 && cin % kKC == 0), "conv3x3: cin must be 3 or a multiple of 16");
  NM_REQUIRE(cout > 0 && cout % kTM == 0, "conv3x3: cout must be a multiple of 64");
  NM_REQUIRE(x && weight && bias && y, "conv3x3: null pointer");
  NM_REQUIRE((cin == 3 || (aligned16(x) && aligned16(weight))) && aligned16(bias) && aligned16(y),
             "conv3x3: pointers must be 16-byte aligned (x and weight: for cin > 3)");
  NM_REQUIRE(x != y, "conv3x3: y may not alias x");
  return conv_launch(n, cin, cout, h, w, x, weight, bias, y, (hipStream_t)stream);
}

extern "C" int nm_maxpool2(int32_t n, int32_t c, int32_t h, int32_t w, const float* x, float* y, void* stream) {
  NM_REQUIRE(n > 0 && h > 0 && w > 0, "maxpool2: n, h and w must be positive");
  NM_REQUIRE(c > 0 && c % 4 == 0, "maxpool2: c must be a multiple of 4");
  NM_REQUIRE(x && y, "maxpool2: null pointer");
  NM_REQUIRE(aligned16(x) && aligned16(y), "maxpool2: pointers must be 16-byte aligned");
  return pool_launch(n, c, h, w, x, y, (hipStream_t)stream);
}

extern "C" size_t nm_lpips_head_workspace(int32_t n_pairs, int32_t h, int32_t w) {
  if (n_pairs <= 0 || h <= 0 || w <= 0) return 0;
  return nm_align256((size_t)n_pairs * head_blocks(h, w) * sizeof(double));
}

extern "C" int nm_lpips_head(int32_t n_pairs, int32_t c, int32_t h, int32_t w, const float* tap_a, const float* tap_b,
                             const float* head_w, double* out_fp64, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(n_pairs > 0 && n_pairs <= 65535 && h > 0 && w > 0, "lpips head: n_pairs in 1..65535, h and w positive");
  NM_REQUIRE((int64_t)h * w < (1 << 30), "lpips head: h * w above 2^30");
  NM_REQUIRE(c > 0 && c % 4 == 0, "lpips head: c must be a multiple of 4");
  NM_REQUIRE(tap_a && tap_b && head_w && out_fp64 && ws, "lpips head: null pointer");
  NM_REQUIRE(aligned16(tap_a) && aligned16(tap_b) && aligned16(head_w), "lpips head: pointers must be 16-byte aligned");
  NM_REQUIRE(ws_bytes >= nm_lpips_head_workspace(n_pairs, h, w), "lpips head: workspace too small (nm_lpips_head_workspace)");
  return head_launch(n_pairs, c, h, w, tap_a, tap_b, head_w, out_fp64, (double*)ws, 0, (hipStream_t)stream);
}

extern "C" size_t nm_lpips_workspace(int32_t b, int32_t h, int32_t w) {
  if (b <= 0 || h < 16 || w < 16) return 0;
  return carve_lpips_ws(nullptr, b, h, w).total;
}

// weights: 26 DEVICE pointers (host array), weight then bias of each convolution in nm_conv3x3_relu's packed layout;
// heads: 5 DEVICE pointers (host array), C floats each.
extern "C" int nm_lpips(int32_t b, int32_t h, int32_t w, const float* a, const float* b_img, const float* const* weights,
                        const float* const* heads, double* out_fp64, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(b > 0 && 2 * (int64_t)b <= 65535, "lpips: b in 1..32767");
  NM_REQUIRE(h >= 16 && w >= 16, "lpips: h and w must be at least 16 (four 2x2 pools)");
  NM_REQUIRE((int64_t)h * w < (1 << 30), "lpips: h * w above 2^30");
  NM_REQUIRE(a && b_img && weights && heads && out_fp64 && ws, "lpips: null pointer");
  for (int i = 0; i < 2 * kConvs; ++i) NM_REQUIRE(weights[i] && aligned16(weights[i]), "lpips: null or unaligned weight pointer");
  for (int i = 0; i < kTaps; ++i) NM_REQUIRE(heads[i] && aligned16(heads[i]), "lpips: null or unaligned head pointer");
  NM_REQUIRE(ws_bytes >= nm_lpips_workspace(b, h, w), "lpips: workspace too small (nm_lpips_workspace)");
  NM_REQUIRE(((uintptr_t)ws & 255) == 0, "lpips: workspace must be 256-byte aligned");
  const LpipsWs W = carve_lpips_ws(ws, b, h, w);
  const hipStream_t s = (hipStream_t)stream;
  const int n = 2 * b;
  NM_LAUNCH(k_lpips_scale, dim3(nm_div_up((int64_t)h * w, 256), n), dim3(256), 0, s, (int)b, (int)h, (int)w, a, b_img, W.scaled);
  NM_LAUNCH_CHECK();
  const float* cur = W.scaled;
  int side = 0, ch = h, cw = w;
  for (int l = 0; l < kConvs; ++l) {
    float* dst = W.act[side];
    int rc = conv_launch(n, kCin[l], kCout[l], ch, cw, cur, weights[2 * l], weights[2 * l + 1], dst, s);
    if (rc != NM_OK) return rc;
    cur = dst; side ^= 1;
    if (kTapAfter[l] >= 0) {
      // the pair's two taps are the two halves of one buffer; it is pooled (or dropped) right after
      rc = head_launch(b, kCout[l], ch, cw, cur, cur + (size_t)b * ch * cw * kCout[l], heads[kTapAfter[l]], out_fp64, W.part,
                       kTapAfter[l] > 0, s);
      if (rc != NM_OK) return rc;
    }
    if (kPoolAfter[l]) {
      dst = W.act[side];
      rc = pool_launch(n, kCout[l], ch, cw, cur, dst, s);
      if (rc != NM_OK) return rc;
      cur = dst; side ^= 1; ch /= 2; cw /= 2;
    }
  }
  return NM_OK;
}
