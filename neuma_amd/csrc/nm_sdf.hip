// Unsigned distance of every node of a regular lattice to a triangle mesh (no reference counterpart; definition:
// include/neuma_hip.h "mesh distance field", the same in numpy - fp64 and fp32 - in neuma_amd/extras/mesh_sdf.py).
//   k_sdf_prep   one thread per triangle: index check and the record the main kernel reads - first vertex, two edges, their
//                three dot products, and a bounding sphere (radius < 0: dropped)
//   k_sdf_dist   one wave per 4x4x4 block of lattice nodes, one lane per node (as the grid sweeps of nm_mpm.hip), four blocks
//                per workgroup.  The records stream through LDS in tiles of 256 that the four waves share; a wave skips a
//                record whose bounding sphere lies farther from the block's bounding sphere than the largest best distance
//                its lanes hold (refreshed every kCullEvery records).  That test is wave-uniform and only prunes: every
//                record that could lower a lane's minimum is evaluated with the full formula.
// The minimum is order-independent and there are no atomics, so two calls give identical bytes.  No host synchronisation.
//
// The per-triangle formula is evaluated as the yardstick's fp32 pass spells it, one rounded operation at a time: no contraction
// into fma (the Makefile passes -ffp-contract=off for this file too), `/` and sqrtf are the correctly rounded ones.
//
// Why the skip cannot change a result.  Let D be the true distance between a node of the block and the triangle, c_b / r_b the
// block's sphere (centre of its 4x4x4 nodes, radius 1.5 sqrt(3) spacing), c_t / r_t the triangle's (centroid, largest vertex
// distance).  Then D >= |c_b - c_t| - r_b - r_t.  Both radii are stored inflated by 1e-4 of themselves plus 1e-5 of the largest
// coordinate magnitude M they were computed from; the rounding of |c_b - c_t|, of the centres and of the evaluated distance
// itself are each a few 2^-24 M ~ 1e-7 M, two orders below that margin.  A record is skipped only when the inflated bound
// exceeds the wave's largest best distance, i.e. when the evaluated distance could not have been smaller for any lane.
#include <math.h>

#include "nm_common.h"
#include "nm_workspace.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSdfThreads = 256;
constexpr int kSdfTile = 256;          // records per LDS tile (64 bytes each: 16 KiB)
constexpr int kCullEvery = 32;         // records between two refreshes of the wave's largest best distance
constexpr int kSdfMaxTris = 1 << 24;
constexpr int64_t kSdfMaxNodes = (int64_t)1 << 27;
constexpr float kDegenerateRel = 1e-6f;      // extras/mesh_sdf.py DEGENERATE_REL

struct SdfRec {       // 16 floats
  float a[3], ab[3], ac[3];
  float aa, bb, cc;   // ab.ab, ab.ac, ac.ac
  float sc[3], sr;    // bounding sphere (inflated radius); sr < 0: dropped triangle
};

struct SdfLattice {
  float o[3];
  float h;
  int n[3];
  int nb[3];          // blocks of 4 per axis
};

__device__ __forceinline__ float dot3(const float x[3], const float y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__global__ void __launch_bounds__(kSdfThreads) k_sdf_prep(int T, int V, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                          SdfRec* __restrict__ rec) {
  const int t = blockIdx.x * kSdfThreads + threadIdx.x;
  if (t >= T) return;
  const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2];
  SdfRec r;
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {      // never read out of range: dropped
    memset(&r, 0, sizeof(r));
    r.sr = -1.f;
    rec[t] = r;
    return;
  }
  float b[3], c[3], cen[3];
  float big = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.a[k] = verts[3 * (size_t)ia + k];
    b[k] = verts[3 * (size_t)ib + k];
    c[k] = verts[3 * (size_t)ic + k];
    r.ab[k] = b[k] - r.a[k];
    r.ac[k] = c[k] - r.a[k];
    cen[k] = (r.a[k] + b[k] + c[k]) * (1.f / 3.f);
    big = fmaxf(big, fmaxf(fabsf(r.a[k]), fmaxf(fabsf(b[k]), fabsf(c[k]))));
  }
  r.aa = dot3(r.ab, r.ab);
  r.bb = dot3(r.ab, r.ac);
  r.cc = dot3(r.ac, r.ac);
  float r2 = 0.f;
  {
    const float da[3] = {r.a[0] - cen[0], r.a[1] - cen[1], r.a[2] - cen[2]};
    const float db[3] = {b[0] - cen[0], b[1] - cen[1], b[2] - cen[2]};
    const float dc[3] = {c[0] - cen[0], c[1] - cen[1], c[2] - cen[2]};
    r2 = fmaxf(dot3(da, da), fmaxf(dot3(db, db), dot3(dc, dc)));
  }
  r.sc[0] = cen[0]; r.sc[1] = cen[1]; r.sc[2] = cen[2];
  const float sr = sqrtf(r2) * (1.f + 1e-4f) + 1e-5f * big;
  r.sr = sr >= 0.f ? sr : INFINITY;                      // (a non-finite vertex: never culled)
  rec[t] = r;
}

// squared distance of p to the segment q0 + t e, t in [0, 1] (a zero-length segment is the point q0)
__device__ __forceinline__ float segment_dist2(const float q0[3], const float e[3], const float p[3]) {
  const float ep[3] = {p[0] - q0[0], p[1] - q0[1], p[2] - q0[2]};
  const float ee = dot3(e, e);
  float t = dot3(e, ep) / (ee > 0.f ? ee : 1.f);
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float d[3] = {ep[0] - e[0] * t, ep[1] - e[1] * t, ep[2] - e[2] * t};
  return dot3(d, d);
}

// squared distance of p to the triangle of record r: the region table of extras/mesh_sdf.py, bottom-up, so that the first
// region that holds wins
__device__ __forceinline__ float triangle_dist2(const SdfRec& r, const float p[3]) {
  if (!(r.aa * r.cc - r.bb * r.bb > kDegenerateRel * (r.aa * r.cc))) {      // wave-uniform: degenerate, the three edge segments
    const float b[3] = {r.a[0] + r.ab[0], r.a[1] + r.ab[1], r.a[2] + r.ab[2]};
    const float bc[3] = {r.ac[0] - r.ab[0], r.ac[1] - r.ab[1], r.ac[2] - r.ab[2]};
    return fminf(fminf(segment_dist2(r.a, r.ab, p), segment_dist2(r.a, r.ac, p)), segment_dist2(b, bc, p));
  }
  const float ap[3] = {p[0] - r.a[0], p[1] - r.a[1], p[2] - r.a[2]};
  const float d1 = dot3(r.ab, ap), d2 = dot3(r.ac, ap);
  const float d3 = d1 - r.aa, d4 = d2 - r.bb, d5 = d1 - r.bb, d6 = d2 - r.cc;
  const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
  const float e43 = d4 - d3, e56 = d5 - d6;
  float nv = vb, nw = vc, den = (va + vb) + vc;
  bool m = va <= 0.f && e43 >= 0.f && e56 >= 0.f;      // edge bc
  nv = m ? e56 : nv; nw = m ? e43 : nw; den = m ? e43 + e56 : den;
  m = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;             // edge ac
  nv = m ? 0.f : nv; nw = m ? d2 : nw; den = m ? d2 - d6 : den;
  m = d6 >= 0.f && d5 <= d6;                           // vertex c
  nv = m ? 0.f : nv; nw = m ? 1.f : nw; den = m ? 1.f : den;
  m = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;             // edge ab
  nv = m ? d1 : nv; nw = m ? 0.f : nw; den = m ? d1 - d3 : den;
  m = d3 >= 0.f && d4 <= d3;                           // vertex b
  nv = m ? 1.f : nv; nw = m ? 0.f : nw; den = m ? 1.f : den;
  m = d1 <= 0.f && d2 <= 0.f;                          // vertex a
  nv = m ? 0.f : nv; nw = m ? 0.f : nw; den = m ? 1.f : den;
  const float rd = 1.f / den;
  const float v = nv * rd, w = nw * rd;
  const float e[3] = {(r.ab[0] * v + r.ac[0] * w) - ap[0], (r.ab[1] * v + r.ac[1] * w) - ap[1], (r.ab[2] * v + r.ac[2] * w) - ap[2]};
  return dot3(e, e);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(kSdfThreads) k_sdf_dist(int T, const SdfRec* __restrict__ rec, SdfLattice L, int n_blocks,
                                                          float* __restrict__ out) {
  __shared__ float4 tile[kSdfTile * 4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int blk_raw = blockIdx.x * 4 + wave;
  const bool live = blk_raw < n_blocks;
  const int blk = live ? blk_raw : n_blocks - 1;      // a spare wave repeats the last block (it shares the tile loads) and stores nothing
  const int bz = blk % L.nb[2], by = (blk / L.nb[2]) % L.nb[1], bx = blk / (L.nb[2] * L.nb[1]);
  const int ix = bx * 4 + (lane >> 4), iy = by * 4 + ((lane >> 2) & 3), iz = bz * 4 + (lane & 3);
  const bool inside = live && ix < L.n[0] && iy < L.n[1] && iz < L.n[2];
  // a lane past the lattice's edge evaluates the edge node instead: its best distance then is some valid lane's, and the
  // wave's largest is not loosened by nodes nobody stores
  const int cx = ix < L.n[0] ? ix : L.n[0] - 1, cy = iy < L.n[1] ? iy : L.n[1] - 1, cz = iz < L.n[2] ? iz : L.n[2] - 1;
  const float p[3] = {L.o[0] + (float)cx * L.h, L.o[1] + (float)cy * L.h, L.o[2] + (float)cz * L.h};
  const float cb[3] = {L.o[0] + ((float)(bx * 4) + 1.5f) * L.h, L.o[1] + ((float)(by * 4) + 1.5f) * L.h,
                       L.o[2] + ((float)(bz * 4) + 1.5f) * L.h};
  const float big = fmaxf(fmaxf(fabsf(cb[0]), fabsf(cb[1])), fabsf(cb[2])) + 2.f * L.h;
  const float rb = 2.5980763f * L.h * (1.f + 1e-4f) + 1e-5f * big;      // 1.5 sqrt(3) h, inflated
  float best = INFINITY;       // squared
  float reach = INFINITY;      // sqrt of the wave's largest best, + rb: a record with |c_b - c_t| > reach + r_t is skipped
  for (int t0 = 0; t0 < T; t0 += kSdfTile) {
    const int nt = T - t0 < kSdfTile ? T - t0 : kSdfTile;
    __syncthreads();
    if ((int)threadIdx.x < nt) {
      const float4* src = (const float4*)(rec + t0 + threadIdx.x);
#pragma unroll
      for (int q = 0; q < 4; ++q) tile[threadIdx.x * 4 + q] = src[q];
    }
    __syncthreads();
    for (int s0 = 0; s0 < nt; s0 += kCullEvery) {
      const int s1 = s0 + kCullEvery < nt ? s0 + kCullEvery : nt;
      for (int s = s0; s < s1; ++s) {
        // a record as four float4: q0 = a.xyz ab.x | q1 = ab.yz ac.xy | q2 = ac.z aa bb cc | q3 = sc.xyz sr (all lanes read the
        // same address: one broadcast read each)
        const float4 q3 = tile[s * 4 + 3];
        const float dx = cb[0] - q3.x, dy = cb[1] - q3.y, dz = cb[2] - q3.z;
        const float dc2 = (dx * dx + dy * dy) + dz * dz;
        const float lim = reach + q3.w;
        const int skip = (q3.w < 0.f) || (dc2 > lim * lim);
        if (__builtin_amdgcn_readfirstlane(skip)) continue;      // every lane computed the same value: one scalar branch
        const float4 q0 = tile[s * 4], q1 = tile[s * 4 + 1], q2 = tile[s * 4 + 2];
        SdfRec r;
        r.a[0] = q0.x; r.a[1] = q0.y; r.a[2] = q0.z;
        r.ab[0] = q0.w; r.ab[1] = q1.x; r.ab[2] = q1.y;
        r.ac[0] = q1.z; r.ac[1] = q1.w; r.ac[2] = q2.x;
        r.aa = q2.y; r.bb = q2.z; r.cc = q2.w;
        best = fminf(best, triangle_dist2(r, p));
      }
      const float worst = wave_max(best);
      reach = sqrtf(worst) * (1.f + 1e-6f) + rb;           // (best = NaN or +inf: reach = +inf or NaN, nothing is skipped)
    }
  }
  if (inside) out[((size_t)ix * L.n[1] + iy) * L.n[2] + iz] = sqrtf(best);
}

bool sdf_sizes_ok(int32_t n_tris, int64_t n_nodes) { return n_tris >= 0 && n_tris <= kSdfMaxTris && n_nodes >= 0 && n_nodes <= kSdfMaxNodes; }

}  // namespace

extern "C" size_t nm_mesh_distance_workspace(int32_t n_tris, int64_t n_nodes) {
  if (!sdf_sizes_ok(n_tris, n_nodes)) return 0;
  NmCarver c(nullptr);
  c.take<SdfRec>(n_tris > 0 ? (size_t)n_tris : 1);
  return c.total();
}

extern "C" int nm_mesh_distance(int32_t n_verts, int32_t n_tris, const float* verts, const int32_t* tris, const float* origin,
                                float spacing, const int32_t* dims, float* dist_out, void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(SdfRec) == 64, "SdfRec is four float4");
  NM_REQUIRE(n_verts >= 0, "n_verts must be >= 0");
  NM_REQUIRE(n_tris >= 0 && n_tris <= kSdfMaxTris, "n_tris must be in [0, 2^24]");
  NM_REQUIRE(origin && dims, "origin and dims must not be NULL");
  NM_REQUIREF(dims[0] >= 2 && dims[1] >= 2 && dims[2] >= 2, "dims: every lattice size must be >= 2 (got %d, %d, %d)", (int)dims[0],
              (int)dims[1], (int)dims[2]);
  const int64_t nodes = (int64_t)dims[0] * dims[1] * dims[2];
  NM_REQUIREF(dims[0] <= kSdfMaxNodes && dims[1] <= kSdfMaxNodes && (int64_t)dims[0] * dims[1] <= kSdfMaxNodes && nodes <= kSdfMaxNodes,
              "dims: %d x %d x %d nodes exceed 2^27", (int)dims[0], (int)dims[1], (int)dims[2]);
  NM_REQUIREF(isfinite(spacing) && spacing > 0.f, "spacing: must be positive and finite (got %g)", (double)spacing);
  NM_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "origin: not finite");
  NM_REQUIRE(dist_out, "dist_out must not be NULL");
  NM_REQUIRE(n_tris == 0 || (tris && (verts || n_verts == 0)), "null pointer");
  NM_REQUIRE(ws && ws_bytes >= nm_mesh_distance_workspace(n_tris, nodes), "workspace too small (nm_mesh_distance_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  SdfRec* rec = c.take<SdfRec>(n_tris > 0 ? (size_t)n_tris : 1);
  if (n_tris > 0) {
    NM_LAUNCH(k_sdf_prep, dim3(nm_div_up(n_tris, kSdfThreads)), dim3(kSdfThreads), 0, s, (int)n_tris, (int)n_verts, verts, tris, rec);
    NM_LAUNCH_CHECK();
  }
  SdfLattice L;
  int64_t n_blocks = 1;
  for (int k = 0; k < 3; ++k) {
    L.o[k] = origin[k];
    L.n[k] = dims[k];
    L.nb[k] = (dims[k] + 3) / 4;
    n_blocks *= L.nb[k];
  }
  L.h = spacing;
  NM_LAUNCH(k_sdf_dist, dim3(nm_div_up(n_blocks, 4)), dim3(kSdfThreads), 0, s, (int)n_tris, (const SdfRec*)rec, L, (int)n_blocks, dist_out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
