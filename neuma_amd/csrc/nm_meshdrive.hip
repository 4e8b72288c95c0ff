// Driven meshes (include/neuma_hip.h "driven meshes"; the definition in numpy fp64: neuma_amd/extras/mesh_drive.py).
//   k_mesh_bind     sixteen lanes per vertex, lane j holding neighbour j.  The k <= 16 neighbours of nm_knn become fixed affine
//                   moving-least-squares coefficients: weights, moments and the damped 3x3 solve in fp64, c_j and w^_j rounded to
//                   fp32 once.  A group's rows of idx, d2, col, coeff and weight are contiguous, so every load and store is
//                   coalesced, each neighbour is gathered and each weight divided once, and nothing is kept per lane but one
//                   neighbour (no run-time-indexed array, no scratch).  The sums over j = 0 .. k-1 run in that order: each is k
//                   broadcasts from lane t = 0, 1, ... that every lane of the group adds up alike; the 3x3 solve is done by all
//                   sixteen lanes redundantly.  (One vertex per lane walking its row four times took 1.70 ms for 655 362
//                   vertices: a lane's row is 128 B from its neighbour's, every 8-byte load of a wave touched 64 lines, and the
//                   rows a CU holds in flight do not fit its L1.)  Runs once per mesh.
//   k_mesh_normals  area-weighted vertex normals without atomics, one pass.  A workgroup owns 256 consecutive vertices, whose
//                   corners are one contiguous stretch of the adjacency (vcorner is sorted by vertex).  The stretch is taken in
//                   chunks of 1024 corners: first every lane computes the cross products of four corners of the chunk, whichever
//                   vertex they belong to - the gathers, which are the cost, are dealt out evenly, so a pole of valence 100 holds
//                   nobody up - and leaves them in LDS; then every lane adds its own vertex's products from LDS in ascending
//                   corner id, which is the order the definition fixes and all that is left serial: three LDS reads and adds per
//                   corner.  Chunks ascend, so the order holds across them.
// Off the training path; no atomics, no host synchronisation: two calls give identical bytes.
#include <math.h>

#include "nm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4 * kThreads;      // corners staged in LDS per trip: 3 x 4 KiB

__device__ __forceinline__ double bind_weight(double d2, double R2) {
  if (!(R2 > 0.0)) return 1.0;
  const double t = 1.0 - d2 / R2;
  return t * t;
}

// a value of lane `src` of the sixteen lanes that share a vertex
__device__ __forceinline__ double group_get(double v, int src) { return __shfl(v, src, 16); }

__global__ void __launch_bounds__(kThreads) k_mesh_bind(int n_verts, int n_particles, int k, double damping,
                                                       const float* __restrict__ verts, const float* __restrict__ particles,
                                                       const int64_t* __restrict__ idx, const double* __restrict__ d2,
                                                       int* __restrict__ col, float* __restrict__ coeff, float* __restrict__ weight) {
  // no lane leaves before the last broadcast: a vertex past the end is computed as the last one and not written, a lane past k
  // stands in for neighbour k - 1 and is never summed
  const int gv = (int)(((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 4);      // (16 V can pass 2^31 where V k does not)
  const int j = threadIdx.x & 15;
  const int v = gv < n_verts ? gv : n_verts - 1;
  const int jj = j < k ? j : k - 1;
  const size_t e = (size_t)v * k + jj;
  const double dj = d2[e];
  // an index nm_knn cannot return (a caller's own list) is never read through: the neighbour counts as particle 0
  const int64_t i64 = idx[e];
  const int i = (i64 >= 0 && i64 < n_particles) ? (int)i64 : 0;
  const double p0 = (double)particles[3 * (size_t)i], p1 = (double)particles[3 * (size_t)i + 1], p2 = (double)particles[3 * (size_t)i + 2];
  const double R2 = 1.21 * group_get(dj, k - 1);
  const double w = bind_weight(dj, R2);
  double W = 0.0;
  for (int t = 0; t < k; ++t) W += group_get(w, t);
  const double wh = w / W;
  // the centroid is summed from the nearest neighbour: Xbar = X_0 + sum w^_j (X_j - X_0).  The differences of fp32 values are
  // exact or nearly so in fp64, so coincident, collinear and coplanar neighbours give moments that vanish exactly where they should
  const double x00 = group_get(p0, 0), x01 = group_get(p1, 0), x02 = group_get(p2, 0);
  const double t0 = wh * (p0 - x00), t1 = wh * (p1 - x01), t2 = wh * (p2 - x02);
  double xb0 = 0.0, xb1 = 0.0, xb2 = 0.0;
  for (int t = 0; t < k; ++t) { xb0 += group_get(t0, t); xb1 += group_get(t1, t); xb2 += group_get(t2, t); }
  xb0 = x00 + xb0; xb1 = x01 + xb1; xb2 = x02 + xb2;
  const double y0 = p0 - xb0, y1 = p1 - xb1, y2 = p2 - xb2;
  const double w0 = wh * y0, w1 = wh * y1, w2 = wh * y2;
  const double q00 = w0 * y0, q01 = w0 * y1, q02 = w0 * y2, q11 = w1 * y1, q12 = w1 * y2, q22 = w2 * y2;
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
  for (int t = 0; t < k; ++t) {
    m00 += group_get(q00, t); m01 += group_get(q01, t); m02 += group_get(q02, t);
    m11 += group_get(q11, t); m12 += group_get(q12, t); m22 += group_get(q22, t);
  }
  const double tau = (m00 + m11) + m22;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  if (tau > 0.0) {
    // (M M + (eps tau)^2 I) g = M r with M^ = M / tau (trace 1): (M^ M^ + eps^2 I) (tau g) = M^ r, solved by L D L^T
    const double h00 = m00 / tau, h01 = m01 / tau, h02 = m02 / tau, h11 = m11 / tau, h12 = m12 / tau, h22 = m22 / tau;
    const double e2 = damping * damping;
    const double a00 = ((h00 * h00 + h01 * h01) + h02 * h02) + e2;
    const double a01 = (h00 * h01 + h01 * h11) + h02 * h12;
    const double a02 = (h00 * h02 + h01 * h12) + h02 * h22;
    const double a11 = ((h01 * h01 + h11 * h11) + h12 * h12) + e2;
    const double a12 = (h01 * h02 + h11 * h12) + h12 * h22;
    const double a22 = ((h02 * h02 + h12 * h12) + h22 * h22) + e2;
    const double r0 = (double)verts[3 * (size_t)v] - xb0, r1 = (double)verts[3 * (size_t)v + 1] - xb1,
                 r2 = (double)verts[3 * (size_t)v + 2] - xb2;
    const double b0 = (h00 * r0 + h01 * r1) + h02 * r2;
    const double b1 = (h01 * r0 + h11 * r1) + h12 * r2;
    const double b2 = (h02 * r0 + h12 * r1) + h22 * r2;
    const double d0 = a00;
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - l10 * a01;
    const double t21 = a12 - l20 * a01;
    const double l21 = t21 / d1;
    const double dd2 = (a22 - l20 * a02) - l21 * t21;
    double z0 = b0;
    double z1 = b1 - l10 * z0;
    double z2 = (b2 - l20 * z0) - l21 * z1;
    z0 /= d0; z1 /= d1; z2 /= dd2;
    const double s2 = z2;
    const double s1 = z1 - l21 * s2;
    const double s0 = (z0 - l10 * s1) - l20 * s2;
    g0 = s0 / tau; g1 = s1 / tau; g2 = s2 / tau;
  }
  if (gv < n_verts && j < k) {
    const double dot = (y0 * g0 + y1 * g1) + y2 * g2;
    col[e] = i;
    coeff[e] = (float)(wh * (1.0 + dot));
    weight[e] = (float)wh;
  }
}

// the cross product corner `cid` = 3 t + c adds to its vertex: (p_next - p_v) x (p_prev - p_v); zero for a corner id outside
// [0, 3 T), a triangle with an index outside [0, V) (never read through) or a repeated index
__device__ __forceinline__ void corner_cross(int cid, int n_verts, int n_tris, const float* __restrict__ pos,
                                             const int* __restrict__ tri, float (&out)[3]) {
  out[0] = out[1] = out[2] = 0.f;
  if (cid < 0 || cid >= 3 * n_tris) return;
  const int t = cid / 3, c = cid - 3 * t;
  const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
  const bool ok = i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts && i0 != i1 && i1 != i2 && i0 != i2;
  if (!ok) return;
  const int iv = c == 0 ? i0 : (c == 1 ? i1 : i2);
  const int in = c == 0 ? i1 : (c == 1 ? i2 : i0);
  const int ip = c == 0 ? i2 : (c == 1 ? i0 : i1);
  const float* pv = pos + 3 * (size_t)iv;
  const float* pn = pos + 3 * (size_t)in;
  const float* pp = pos + 3 * (size_t)ip;
  const float a0 = pn[0] - pv[0], a1 = pn[1] - pv[1], a2 = pn[2] - pv[2];
  const float b0 = pp[0] - pv[0], b1 = pp[1] - pv[1], b2 = pp[2] - pv[2];
  out[0] = a1 * b2 - a2 * b1;
  out[1] = a2 * b0 - a0 * b2;
  out[2] = a0 * b1 - a1 * b0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kThreads) k_mesh_normals(int n_verts, int n_tris, const float* __restrict__ pos,
                                                          const int* __restrict__ tri, const int* __restrict__ vptr,
                                                          const int* __restrict__ vcorner, float* __restrict__ normals) {
  __shared__ float sh[3][kChunk];
  const int v0 = blockIdx.x * kThreads;
  const int v = v0 + threadIdx.x;
  const int v1 = v0 + kThreads < n_verts ? v0 + kThreads : n_verts;
  const int nc = 3 * n_tris;
  // (every bound is clamped into [0, 3 T]: an adjacency that is not what corner_adjacency builds can give wrong normals, never a
  //  read outside the arrays)
  const int lo = clampi(vptr[v0], 0, nc), hi = clampi(vptr[v1], 0, nc);     // the workgroup's stretch: the same in every lane
  int mine0 = 0, mine1 = 0;
  if (v < n_verts) { mine0 = clampi(vptr[v], 0, nc); mine1 = clampi(vptr[v + 1], 0, nc); }
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int base = lo; base < hi; base += kChunk) {
    const int end = base + kChunk < hi ? base + kChunk : hi;
#pragma unroll
    for (int u = 0; u < kChunk / kThreads; ++u) {
      const int q = base + u * kThreads + threadIdx.x;
      if (q < end) {
        float x[3];
        corner_cross(vcorner[q], n_verts, n_tris, pos, tri, x);
        sh[0][q - base] = x[0]; sh[1][q - base] = x[1]; sh[2][q - base] = x[2];
      }
    }
    __syncthreads();
    const int a = mine0 > base ? mine0 : base, b = mine1 < end ? mine1 : end;
    for (int q = a; q < b; ++q) { s0 += sh[0][q - base]; s1 += sh[1][q - base]; s2 += sh[2][q - base]; }
    __syncthreads();
  }
  if (v >= n_verts) return;
  const float m = fmaxf(fmaxf(fabsf(s0), fabsf(s1)), fabsf(s2));
  float n0 = 0.f, n1 = 0.f, n2 = 0.f;
  if (m > 0.f && m <= 3.402823466e+38f && s0 == s0 && s1 == s1 && s2 == s2) {
    const float t0 = s0 / m, t1 = s1 / m, t2 = s2 / m;
    const float len = sqrtf((t0 * t0 + t1 * t1) + t2 * t2);
    n0 = t0 / len; n1 = t1 / len; n2 = t2 / len;
  }
  normals[3 * (size_t)v] = n0; normals[3 * (size_t)v + 1] = n1; normals[3 * (size_t)v + 2] = n2;
}

}  // namespace

extern "C" int nm_mesh_bind(int32_t n_verts, int32_t n_particles, int32_t k, double damping, const float* verts,
                            const float* particles, const int64_t* idx, const double* d2, int32_t* col, float* coeff,
                            float* weight, void* stream) {
  NM_REQUIREF(k >= 1 && k <= 16, "k = %d outside 1..16", (int)k);
  NM_REQUIREF(n_verts >= 0 && n_particles >= k, "n_verts = %d < 0 or n_particles = %d < k = %d", (int)n_verts, (int)n_particles, (int)k);
  NM_REQUIREF((int64_t)n_verts * k < ((int64_t)1 << 31), "n_verts k = %lld does not fit an int32", (long long)n_verts * k);
  NM_REQUIREF(damping > 0.0 && damping < (double)INFINITY, "damping = %g must be finite and > 0", damping);
  if (n_verts == 0) return NM_OK;
  NM_REQUIRE(verts && particles && idx && d2 && col && coeff && weight, "null pointer");
  NM_LAUNCH(k_mesh_bind, dim3(nm_div_up((int64_t)n_verts * 16, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n_verts, (int)n_particles, (int)k,
            damping, verts, particles, idx, d2, col, coeff, weight);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_mesh_normals(int32_t n_verts, int32_t n_tris, const float* positions, const int32_t* triangles, const int32_t* vptr,
                               const int32_t* vcorner, float* normals_out, void* stream) {
  NM_REQUIREF(n_verts >= 0 && n_tris >= 0, "n_verts = %d < 0 or n_tris = %d < 0", (int)n_verts, (int)n_tris);
  NM_REQUIREF((int64_t)n_tris * 3 < ((int64_t)1 << 31), "3 n_tris = %lld does not fit an int32", 3LL * n_tris);
  if (n_verts == 0) return NM_OK;
  NM_REQUIRE(positions && vptr && normals_out, "null pointer");
  NM_REQUIRE(n_tris == 0 || (triangles && vcorner), "triangles and vcorner must not be NULL with n_tris > 0");
  NM_LAUNCH(k_mesh_normals, dim3(nm_div_up(n_verts, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (int)n_verts, (int)n_tris, positions,
            triangles, vptr, vcorner, normals_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
