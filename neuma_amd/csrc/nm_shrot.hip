// Rotation of SH colour coefficients with the Gaussians (transform_shs_by_rotmat of the reference's transform_utils.py) and
// its adjoint.  c' = diag(1, D_1, D_2, D_3) c per Gaussian and colour channel, D defined by
//   sum_j c'_j Y_j(R d) = sum_j c_j Y_j(d)   for every unit d,     Y_j = the basis k_preprocess (nm_raster.hip) evaluates.
// Each Y_l is a homogeneous polynomial of degree l, so with 2l+1 fixed directions s_k
//   D_l = [Y_l(R s_1) ... Y_l(R s_{2l+1})] A_l^{-1},   A_l = [Y_l(s_k)] a constant:
// a polynomial in the entries of R, no angles.  The same formula, directions and A_l^{-1} as sh_rotation_matrices of
// neuma_amd/render/transform_utils.py (tools/gen_shrot_tables.py writes the table below from it).
//   nm_sh_rotate           D (<= 83 entries) once per workgroup in fp64 into LDS; 64 Gaussians per tile staged through LDS:
//                          global loads and stores run over consecutive floats, each lane then owns one (Gaussian, channel)
//   nm_sh_rotate_backward  dD = sum_K dL_dout (x) in: every D entry has ONE owning lane per channel that walks the tile in
//                          LDS with an fp64 accumulator (no cross-lane step is needed), one partial set per workgroup, then
//                          one workgroup sums them in a fixed order and chains dD -> dR.  No atomics: bitwise reproducible.
//   nm_sh_rotate_polar     one rotation PER Gaussian, the polar factor of its deformation gradient: nm_svd3 one Gaussian per
//                          lane, then c'_l = Y_l(R s_k) (A_l^{-1} c_l) per (Gaussian, channel) lane; D_l is never formed.
#include "nm_common.h"

namespace {

// BEGIN generated tables (tools/gen_shrot_tables.py)
// unit sample directions s_k; band l uses the first 2l+1
#define NM_SHROT_DIRS \
    -0.7071067811865475, -0.7071067811865475, 0.0, \
    0.0, -0.7071067811865476, 0.7071067811865476, \
    -0.7276068751089989, 0.48507125007266594, 0.48507125007266594, \
    1.0, 0.0, 0.0, \
    0.6666666666666666, -0.6666666666666666, 0.3333333333333333, \
    -0.2672612419124244, -0.5345224838248488, -0.8017837257372732, \
    -0.6396021490668313, -0.6396021490668313, -0.42640143271122083
// A_1^{-1} (3x3) | A_2^{-1} (5x5) | A_3^{-1} (7x7), each row-major [k][j], A_l[i][k] = Y_l,i(s_k)
#define NM_SHROT_AINV \
    1.240459293528459, -1.2404592935284593, 1.6539457247046119, \
    0.8269728623523058, 2.067432155880765, -0.8269728623523058, \
    -1.205509744679705, 1.205509744679705, 1.205509744679705, \
    0.6101941552425129, 0.0, -2.113774558723206, 0.6101941552425127, -1.2203883104850255, \
    0.13559870116500278, 1.8305824657275374, 0.23486383985813394, 1.3559870116500279, 0.13559870116500278, \
    -0.5762944799512619, 0.0, -0.9981713193970694, 2.017030679829417, -0.5762944799512618, \
    0.23729772703875493, 0.9152912328637689, 0.41101171975173445, 0.08474918822812674, 2.067880192766293, \
    -0.915291232863769, -0.0, -1.5853309190424043, -0.915291232863769, -0.9152912328637689, \
    0.7964968437591189, 0.2903644094765842, 0.3162221843112834, -1.225273298365035, -1.191099149832384, 0.29119043517933696, -0.9226214341965266, \
    -0.09033283828889813, -0.21499957101966888, 0.5159172330381264, -0.45341031234184354, -0.3162682129038217, -1.313584644643325, -0.24498030430225645, \
    -1.055236213275335, -0.7457643212036495, -0.4764392828762665, -0.5427411324452068, -0.44293240528359185, 0.11894354772280692, -0.34309396583178864, \
    0.02365176192399859, 0.2299069624258697, -0.5076589442947648, -0.19818355265759563, 1.363078886212459, -0.4400925796679911, -0.6389536758881907, \
    0.8689062196106156, -0.3268707789702451, -0.28472229247202463, -0.7628078663536809, 0.703237699230672, -0.4278846179973939, 0.5447255795091229, \
    0.6903580885547285, 0.1768392216221918, 1.4572828716484794, -0.4823500860642566, -0.28301720584223183, 1.225204668098874, -0.2192241849834241, \
    -0.15560168619469703, -1.0898004610995478, -0.24748024716261752, 1.4972479661796438, 0.02329966703566649, -0.5578440172420881, 0.018047844480262736
// END generated tables

constexpr int kShTile = 64;        // Gaussians per tile
constexpr int kShThreads = 256;
constexpr int kShMaxBlocks = 1024;
constexpr int kShND = 83;          // 9 + 25 + 49

NM_HD double sh_dir(int k, int a) {
  const double t[7][3] = {NM_SHROT_DIRS};
  return t[k][a];
}
NM_HD double sh_ainv(int e) {
  const double t[kShND] = {NM_SHROT_AINV};
  return t[e];
}

NM_HD constexpr int band_n(int l) { return 2 * l + 1; }
NM_HD constexpr int band_row(int l) { return l * l - 1; }                              // first row of band l below the DC row: 0, 3, 8
NM_HD constexpr int band_off(int l) { return l == 1 ? 0 : (l == 2 ? 9 : 34); }          // first entry of D_l among the 83
NM_HD constexpr int deg_entries(int deg) { return deg == 1 ? 9 : (deg == 2 ? 34 : 83); }
NM_HD constexpr int deg_of_rows(int nr) { return nr == 3 ? 1 : (nr == 8 ? 2 : 3); }

constexpr double kC1 = 0.4886025119029199;
constexpr double kC2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
constexpr double kC3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                           -0.4570457994644658, 1.445305721320277,  -0.5900435899266435};

// Y_l (2l+1 values) at p, as homogeneous polynomials: p is not normalised
NM_HD void sh_band(int l, const double* p, double* Y) {
  const double x = p[0], y = p[1], z = p[2];
  if (l == 1) {
    Y[0] = -kC1 * y; Y[1] = kC1 * z; Y[2] = -kC1 * x;
    return;
  }
  const double xx = x * x, yy = y * y, zz = z * z;
  if (l == 2) {
    Y[0] = kC2[0] * (x * y); Y[1] = kC2[1] * (y * z); Y[2] = kC2[2] * (2.0 * zz - xx - yy); Y[3] = kC2[3] * (x * z);
    Y[4] = kC2[4] * (xx - yy);
    return;
  }
  Y[0] = kC3[0] * y * (3.0 * xx - yy);
  Y[1] = kC3[1] * (x * y) * z;
  Y[2] = kC3[2] * y * (4.0 * zz - xx - yy);
  Y[3] = kC3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
  Y[4] = kC3[4] * x * (4.0 * zz - xx - yy);
  Y[5] = kC3[5] * z * (xx - yy);
  Y[6] = kC3[6] * x * (xx - 3.0 * yy);
}

// g[a] = sum_i w[i] dY_l,i/dp_a
NM_HD void sh_band_adj(int l, const double* p, const double* w, double* g) {
  const double x = p[0], y = p[1], z = p[2];
  if (l == 1) {
    g[0] = -kC1 * w[2]; g[1] = -kC1 * w[0]; g[2] = kC1 * w[1];
    return;
  }
  if (l == 2) {
    const double a0 = kC2[0] * w[0], a1 = kC2[1] * w[1], a2 = kC2[2] * w[2], a3 = kC2[3] * w[3], a4 = kC2[4] * w[4];
    g[0] = a0 * y - 2.0 * a2 * x + a3 * z + 2.0 * a4 * x;
    g[1] = a0 * x + a1 * z - 2.0 * a2 * y - 2.0 * a4 * y;
    g[2] = a1 * y + 4.0 * a2 * z + a3 * x;
    return;
  }
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
  const double b0 = kC3[0] * w[0], b1 = kC3[1] * w[1], b2 = kC3[2] * w[2], b3 = kC3[3] * w[3], b4 = kC3[4] * w[4],
               b5 = kC3[5] * w[5], b6 = kC3[6] * w[6];
  g[0] = 6.0 * b0 * xy + b1 * yz - 2.0 * b2 * xy - 6.0 * b3 * xz + b4 * (4.0 * zz - 3.0 * xx - yy) + 2.0 * b5 * xz +
         3.0 * b6 * (xx - yy);
  g[1] = 3.0 * b0 * (xx - yy) + b1 * xz + b2 * (4.0 * zz - xx - 3.0 * yy) - 6.0 * b3 * yz - 2.0 * b4 * xy - 2.0 * b5 * yz -
         6.0 * b6 * xy;
  g[2] = b1 * xy + 8.0 * b2 * yz + 3.0 * b3 * (2.0 * zz - xx - yy) + 8.0 * b4 * xz + b5 * (xx - yy);
}

// p = R s_k
NM_HD void sh_sample_point(const float* __restrict__ R, int k, double* p) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    p[a] = (double)R[3 * a] * sh_dir(k, 0) + (double)R[3 * a + 1] * sh_dir(k, 1) + (double)R[3 * a + 2] * sh_dir(k, 2);
}

// (band, index within the band) of sample row r = band_row(l) + k, 0 <= r < 15
NM_HD int row_band(int r) { return r < 3 ? 1 : (r < 8 ? 2 : 3); }
// band of entry e, 0 <= e < 83
NM_HD int entry_band(int e) { return e < 9 ? 1 : (e < 34 ? 2 : 3); }

// D[e] = sum_k Y_l,i(R s_k) A_l^{-1}[k][j] for entry e = band_off(l) + i n + j, from the sampled yv[band_row(l) + k][i]
NM_HD double sh_D_entry(int e, const double (*yv)[7]) {
  const int l = entry_band(e), n = band_n(l), q = e - band_off(l), i = q / n, j = q % n;
  double v = 0.0;
  for (int k = 0; k < n; ++k) v += yv[band_row(l) + k][i] * sh_ainv(band_off(l) + k * n + j);
  return v;
}

// All threads of the workgroup: D (deg_entries(deg) floats) from the nine DEVICE floats of R.  Ends with a barrier.
__device__ __forceinline__ void build_D(int deg, const float* __restrict__ R, double (*yv)[7], float* __restrict__ D) {
  const int t = threadIdx.x;
  if (t < deg * (deg + 2)) {
    double p[3];
    const int l = row_band(t);
    sh_sample_point(R, t - band_row(l), p);
    sh_band(l, p, yv[t]);
  }
  __syncthreads();
  if (t < deg_entries(deg)) D[t] = (float)sh_D_entry(t, yv);
  __syncthreads();
}

// tile <-> global over consecutive floats (16-byte accesses when both ends allow); rows of S floats sit P apart in LDS
template <int S, int P, bool kStore>
__device__ __forceinline__ void tile_copy(float* tile, float* g, int cnt, bool vec) {
  const int t = threadIdx.x;
  int done = 0;
  if (vec) {
    const int n4 = cnt >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    for (int q = t; q < n4; q += kShThreads) {
      const int e = 4 * q;
      const int o0 = (e / S) * P + e % S, o1 = ((e + 1) / S) * P + (e + 1) % S, o2 = ((e + 2) / S) * P + (e + 2) % S,
                o3 = ((e + 3) / S) * P + (e + 3) % S;
      if (kStore) {
        g4[q] = make_float4(tile[o0], tile[o1], tile[o2], tile[o3]);
      } else {
        const float4 v = g4[q];
        tile[o0] = v.x; tile[o1] = v.y; tile[o2] = v.z; tile[o3] = v.w;
      }
    }
    done = n4 << 2;
  }
  for (int e = done + t; e < cnt; e += kShThreads) {
    const int o = (e / S) * P + e % S;
    if (kStore) g[e] = tile[o];
    else tile[o] = g[e];
  }
}

// one (Gaussian, channel): c[3 j] <- sum D (kT: D^T) c over each band, in place.  c points at the first non-DC row.
template <int DEG, bool kT>
__device__ __forceinline__ void rotate_item(float* __restrict__ c, const float* __restrict__ D) {
  constexpr int NR = DEG * (DEG + 2);
  float v[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) v[j] = c[3 * j];
#pragma unroll
  for (int l = 1; l <= DEG; ++l) {
    const int n = band_n(l), r0 = band_row(l), o = band_off(l);
#pragma unroll
    for (int i = 0; i < n; ++i) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < n; ++j) s += (kT ? D[o + j * n + i] : D[o + i * n + j]) * v[r0 + j];
      c[3 * (r0 + i)] = s;
    }
  }
}

template <int NR, int DC>
__global__ void __launch_bounds__(kShThreads) k_sh_rotate(int K, const float* __restrict__ R, const float* in, float* out /* may be in */,
                                                          int vec) {
  constexpr int S = 3 * (NR + DC), P = S | 1, DEG = deg_of_rows(NR);
  __shared__ double yv[15][7];
  __shared__ float D[kShND];
  __shared__ float tile[kShTile * P];
  build_D(DEG, R, yv, D);
  const int ntiles = (K + kShTile - 1) / kShTile;
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int g0 = ti * kShTile, ng = min(kShTile, K - g0);
    const size_t base = (size_t)g0 * S;
    tile_copy<S, P, false>(tile, const_cast<float*>(in) + base, ng * S, vec);
    __syncthreads();
    if (threadIdx.x < 3 * kShTile) {
      const int ch = threadIdx.x / kShTile, g = threadIdx.x % kShTile;      // one channel per wave: rows P (odd) apart, no bank conflict
      if (g < ng) rotate_item<DEG, false>(tile + g * P + 3 * DC + ch, D);
    }
    __syncthreads();
    tile_copy<S, P, true>(tile, out + base, ng * S, vec);
    __syncthreads();
  }
}

template <int NR, int DC>
__global__ void __launch_bounds__(kShThreads) k_sh_rotate_bwd(int K, const float* __restrict__ R, const float* __restrict__ in,
                                                              const float* gout, float* gin /* NULL, or may be gout */,
                                                              double* __restrict__ part, int vec) {
  constexpr int S = 3 * (NR + DC), P = S | 1, DEG = deg_of_rows(NR), NE = deg_entries(DEG);
  __shared__ double yv[15][7];
  __shared__ float D[kShND];
  __shared__ float tc[kShTile * P], tg[kShTile * P];
  __shared__ double red[3 * NE];
  if (gin) build_D(DEG, R, yv, D);                    // (uniform: a kernel argument)
  const int t = threadIdx.x;
  const bool owner = t < 3 * NE;                      // lane (channel, entry): dD[e] of that channel
  int oi = 0, oj = 0;
  if (owner) {
    const int ch = t / NE, e = t % NE, l = entry_band(e), n = band_n(l), q = e - band_off(l);
    oi = 3 * (DC + band_row(l) + q / n) + ch;
    oj = 3 * (DC + band_row(l) + q % n) + ch;
  }
  double acc = 0.0;
  const int ntiles = (K + kShTile - 1) / kShTile;
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int g0 = ti * kShTile, ng = min(kShTile, K - g0);
    const size_t base = (size_t)g0 * S;
    tile_copy<S, P, false>(tc, const_cast<float*>(in) + base, ng * S, vec);
    tile_copy<S, P, false>(tg, const_cast<float*>(gout) + base, ng * S, vec);
    __syncthreads();
    if (owner)
      for (int g = 0; g < ng; ++g) acc += (double)tg[g * P + oi] * (double)tc[g * P + oj];     // a row: < 64 distinct words
    if (gin) {
      __syncthreads();
      if (t < 3 * kShTile) {
        const int ch = t / kShTile, g = t % kShTile;
        if (g < ng) rotate_item<DEG, true>(tg + g * P + 3 * DC + ch, D);                       // D^T dL_dout; the DC row passes
      }
      __syncthreads();
      tile_copy<S, P, true>(tg, gin + base, ng * S, vec);
    }
    __syncthreads();
  }
  if (owner) red[t] = acc;
  __syncthreads();
  if (t < NE) part[(size_t)blockIdx.x * NE + t] = (red[t] + red[NE + t]) + red[2 * NE + t];
}

// band L of one (Gaussian, channel) rotated in place by the Gaussian's own R (nine floats) without forming D_l:
//   w = A_l^{-1} c_l,   c'_l,i = sum_k Y_l,i(R s_k) w_k.   Everything between the fp32 load and the fp32 store is fp64.
template <int L>
NM_HD void rotate_band_polar(float* __restrict__ c, const float* __restrict__ R) {
  constexpr int n = band_n(L), r0 = band_row(L), o = band_off(L);
  double v[n], acc[n];
#pragma unroll
  for (int j = 0; j < n; ++j) { v[j] = (double)c[3 * (r0 + j)]; acc[j] = 0.0; }
#pragma unroll
  for (int k = 0; k < n; ++k) {
    double p[3], Y[n], w = 0.0;
    sh_sample_point(R, k, p);
    sh_band(L, p, Y);
#pragma unroll
    for (int j = 0; j < n; ++j) w += sh_ainv(o + k * n + j) * v[j];
#pragma unroll
    for (int i = 0; i < n; ++i) acc[i] += Y[i] * w;
  }
#pragma unroll
  for (int i = 0; i < n; ++i) c[3 * (r0 + i)] = (float)acc[i];
}

// K different rotations: R_k = U V^T of nm_svd3(F_k), the rotation of the polar decomposition (proper also where det F < 0).
// Per tile of 64 Gaussians: coefficient rows and F staged through LDS over consecutive floats; the first wave takes one SVD per
// lane and leaves R where F was (row stride 9: odd, no bank conflict); three waves then own one (Gaussian, channel) each, one
// channel per wave (rows P, odd, apart).  A Gaussian's result depends on nothing but its own row: not on the tile, not on K.
template <int NR, int DC>
__global__ void __launch_bounds__(kShThreads) k_sh_rotate_polar(int K, const float* __restrict__ F, const float* in,
                                                                float* __restrict__ out, float* __restrict__ R_out /* or NULL */,
                                                                int vec) {
  constexpr int S = 3 * (NR + DC), P = S | 1, DEG = deg_of_rows(NR);
  __shared__ float tile[kShTile * P];
  __shared__ float rot[kShTile * 9];
  const int t = threadIdx.x;
  const int ntiles = (K + kShTile - 1) / kShTile;
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int g0 = ti * kShTile, ng = min(kShTile, K - g0);
    const size_t base = (size_t)g0 * S, fbase = (size_t)g0 * 9;
    tile_copy<S, P, false>(tile, const_cast<float*>(in) + base, ng * S, vec);
    for (int e = t; e < ng * 9; e += kShThreads) rot[e] = F[fbase + e];
    __syncthreads();
    if (t < ng) {
      M3 U, V;
      float s[3];
      nm_svd3(m3_load(rot + 9 * t), U, s, V);
      m3_store(rot + 9 * t, m3_mul_nt(U, V));
    }
    __syncthreads();
    if (t < 3 * kShTile) {
      const int ch = t / kShTile, g = t % kShTile;
      if (g < ng) {
        float* c = tile + g * P + 3 * DC + ch;
        const float* R = rot + 9 * g;
        rotate_band_polar<1>(c, R);
        if (DEG >= 2) rotate_band_polar<2>(c, R);
        if (DEG >= 3) rotate_band_polar<3>(c, R);
      }
    }
    if (R_out)                                              // (uniform: a kernel argument)
      for (int e = t; e < ng * 9; e += kShThreads) R_out[fbase + e] = rot[e];
    __syncthreads();
    tile_copy<S, P, true>(tile, out + base, ng * S, vec);
    __syncthreads();
  }
}

// one workgroup: dD = the partials in a fixed order, then dR[a][b] += sum_{l,k} (dY_l/dp (R s_k) . (dD_l A_l^{-T})[:, k])_a s_k[b]
__global__ void __launch_bounds__(kShThreads) k_sh_rotate_finish(int deg, int nb, const float* __restrict__ R,
                                                                 const double* __restrict__ part, float* __restrict__ dR) {
  __shared__ double red[2][kShND];
  __shared__ double dD[kShND];
  __shared__ double gp[15][3];
  const int t = threadIdx.x, ne = deg_entries(deg);
  const int e = t & 127, half = t >> 7;
  if (e < ne) {
    double acc = 0.0;
    for (int b = half; b < nb; b += 2) acc += part[(size_t)b * ne + e];
    red[half][e] = acc;
  }
  __syncthreads();
  if (t < ne) dD[t] = red[0][t] + red[1][t];
  __syncthreads();
  const int nrow = deg * (deg + 2);
  if (t < nrow) {
    const int l = row_band(t), n = band_n(l), k = t - band_row(l);
    double p[3], w[7];
    sh_sample_point(R, k, p);
    for (int i = 0; i < n; ++i) {
      double v = 0.0;
      for (int j = 0; j < n; ++j) v += dD[band_off(l) + i * n + j] * sh_ainv(band_off(l) + k * n + j);
      w[i] = v;
    }
    sh_band_adj(l, p, w, gp[t]);
  }
  __syncthreads();
  if (t < 9) {
    const int a = t / 3, b = t % 3;
    double v = 0.0;
    for (int r = 0; r < nrow; ++r) v += gp[r][a] * sh_dir(r - band_row(row_band(r)), b);
    dR[t] = (float)((double)dR[t] + v);
  }
}

int sh_blocks(int k) {
  const int b = nm_div_up(k, kShTile);
  return b < 1 ? 1 : (b > kShMaxBlocks ? kShMaxBlocks : b);
}

// rows below the DC row, or 0 for a count the basis does not have
int sh_rest_rows(int32_t n_coeff, int32_t has_dc) {
  const int nr = n_coeff - (has_dc ? 1 : 0);
  return (nr == 3 || nr == 8 || nr == 15) ? nr : 0;
}

}  // namespace

#define NM_SH_DISPATCH(KERN, nr, dc, ...)                                                          \
  do {                                                                                             \
    if (nr == 3 && !dc) NM_LAUNCH((KERN<3, 0>), __VA_ARGS__);                                      \
    else if (nr == 3) NM_LAUNCH((KERN<3, 1>), __VA_ARGS__);                                        \
    else if (nr == 8 && !dc) NM_LAUNCH((KERN<8, 0>), __VA_ARGS__);                                 \
    else if (nr == 8) NM_LAUNCH((KERN<8, 1>), __VA_ARGS__);                                        \
    else if (!dc) NM_LAUNCH((KERN<15, 0>), __VA_ARGS__);                                           \
    else NM_LAUNCH((KERN<15, 1>), __VA_ARGS__);                                                    \
  } while (0)

extern "C" int nm_sh_rotate(int32_t k, int32_t n_coeff, int32_t has_dc, const float* R, const float* shs_in, float* shs_out,
                            void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  const int nr = sh_rest_rows(n_coeff, has_dc);
  NM_REQUIRE(nr != 0, "n_coeff must be 4, 9, 16 with has_dc = 1 or 3, 8, 15 with has_dc = 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(R && shs_in && shs_out, "null pointer");
  const int dc = has_dc ? 1 : 0;
  const int vec = (((uintptr_t)shs_in | (uintptr_t)shs_out) % 16 == 0) ? 1 : 0;
  NM_SH_DISPATCH(k_sh_rotate, nr, dc, dim3(sh_blocks(k)), dim3(kShThreads), 0, (hipStream_t)stream, (int)k, R, shs_in, shs_out, vec);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_sh_rotate_polar(int32_t k, int32_t n_coeff, int32_t has_dc, const float* F, const float* shs_in, float* shs_out,
                                  float* R_out, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  const int nr = sh_rest_rows(n_coeff, has_dc);
  NM_REQUIRE(nr != 0, "n_coeff must be 4, 9, 16 with has_dc = 1 or 3, 8, 15 with has_dc = 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(F && shs_in && shs_out, "null pointer");
  NM_REQUIRE(shs_out != shs_in, "shs_out must not be shs_in");
  const int dc = has_dc ? 1 : 0;
  const int vec = (((uintptr_t)shs_in | (uintptr_t)shs_out) % 16 == 0) ? 1 : 0;
  NM_SH_DISPATCH(k_sh_rotate_polar, nr, dc, dim3(sh_blocks(k)), dim3(kShThreads), 0, (hipStream_t)stream, (int)k, F, shs_in, shs_out,
                 R_out, vec);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" size_t nm_sh_rotate_bwd_workspace(int32_t k) {
  return (size_t)sh_blocks(k < 0 ? 0 : k) * kShND * sizeof(double);
}

extern "C" int nm_sh_rotate_backward(int32_t k, int32_t n_coeff, int32_t has_dc, const float* R, const float* shs_in,
                                     const float* dL_dshs_out, float* dL_dR, float* dL_dshs_in, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  NM_REQUIRE(k >= 0, "k < 0");
  const int nr = sh_rest_rows(n_coeff, has_dc);
  NM_REQUIRE(nr != 0, "n_coeff must be 4, 9, 16 with has_dc = 1 or 3, 8, 15 with has_dc = 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(R && shs_in && dL_dshs_out && dL_dR && workspace, "null pointer");
  NM_REQUIRE(workspace_bytes >= nm_sh_rotate_bwd_workspace(k), "workspace too small (nm_sh_rotate_bwd_workspace)");
  const int dc = has_dc ? 1 : 0, nb = sh_blocks(k);
  const int vec = (((uintptr_t)shs_in | (uintptr_t)dL_dshs_out | (uintptr_t)dL_dshs_in) % 16 == 0) ? 1 : 0;
  double* part = (double*)workspace;
  NM_SH_DISPATCH(k_sh_rotate_bwd, nr, dc, dim3(nb), dim3(kShThreads), 0, (hipStream_t)stream, (int)k, R, shs_in, dL_dshs_out,
                 dL_dshs_in, part, vec);
  NM_LAUNCH_CHECK();
  NM_LAUNCH(k_sh_rotate_finish, dim3(1), dim3(kShThreads), 0, (hipStream_t)stream, deg_of_rows(nr), nb, R, (const double*)part,
            dL_dR);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
