// Ray / segment versus the DRAWN SOLID of a collider (definition: include/neuma_hip.h "Drawing colliders", fp64 yardstick:
// neuma_amd/extras/collider_draw.py, which spells the same operations in the same order).  The drawn solid is the collider's
// shape cut by the unit cube [0,1]^3 - both convex, so the points o + t d inside it form one open interval (t_in, t_out): the
// intersection of the intervals of the single constraints.  Each constraint has the form lo < q + t dq < hi (ray_slab) or is the
// sphere's quadratic; t_in is the largest entry, t_out the smallest exit, and the interval is empty when t_in >= t_out.
//   which   the constraint that produced t_in: 0..2 the shape (plane face / sphere: 0; box: its axis), 3..5 the cube's axis
//           (strict >: of equal entries the first in the order shape, cube x, y, z stays)
//   n       with WANT_N the outward normal there in simulation coordinates, not normalised (sphere: p - centre)
// d need not be a unit vector: the pixel kernel passes the render-space unit direction divided by the per-axis scale, the
// Gaussian kernel the whole segment camera -> mean (t in 0..1).  No arrays indexed at run time: everything is unrolled.
#pragma once
#include "nm_common.h"

#define NM_RAY_INF __builtin_huge_valf()

// lo < q + t dq < hi  ->  (t0, t1); dq = 0: everything or nothing
__device__ __forceinline__ void ray_slab(float q, float dq, float lo, float hi, float& t0, float& t1) {
  const bool fwd = dq > 0.f, still = dq == 0.f;
  const float inv = 1.f / (still ? 1.f : dq);      // one division per pair of faces
  const float a = ((fwd ? lo : hi) - q) * inv;
  const float b = ((fwd ? hi : lo) - q) * inv;
  const bool in = q > lo && q < hi;
  t0 = still ? (in ? -NM_RAY_INF : NM_RAY_INF) : a;
  t1 = still ? (in ? NM_RAY_INF : -NM_RAY_INF) : b;
}

// the unit cube's three slabs: the same for every collider, so a kernel computes them once per ray
struct RayCube {
  float t0[3], t1[3];
};
__device__ __forceinline__ RayCube ray_cube(const float o[3], const float d[3]) {
  RayCube k;
#pragma unroll
  for (int a = 0; a < 3; ++a) ray_slab(o[a], d[a], 0.f, 1.f, k.t0[a], k.t1[a]);
  return k;
}

template <bool WANT_N>
__device__ __forceinline__ void ray_solid(const nm_collider& c, const float o[3], const float d[3], const RayCube& cube, float& t_in,
                                          float& t_out, int& which, float n[3]) {
  const float m[3] = {o[0] - c.center[0], o[1] - c.center[1], o[2] - c.center[2]};
  which = 0;
  if (c.shape == NM_COLLIDER_PLANE) {
    const float s0 = c.normal[0] * m[0] + c.normal[1] * m[1] + c.normal[2] * m[2];
    const float sd = c.normal[0] * d[0] + c.normal[1] * d[1] + c.normal[2] * d[2];
    const float tt = -s0 / (sd == 0.f ? 1.f : sd);
    const bool in = s0 < 0.f;
    t_in = sd < 0.f ? tt : ((sd > 0.f || in) ? -NM_RAY_INF : NM_RAY_INF);
    t_out = sd > 0.f ? tt : ((sd < 0.f || in) ? NM_RAY_INF : -NM_RAY_INF);
    if (WANT_N) { n[0] = c.normal[0]; n[1] = c.normal[1]; n[2] = c.normal[2]; }
  } else if (c.shape == NM_COLLIDER_SPHERE) {
    // with q the offset of the centre from the line: inside while |q|^2 + A (t + b/A)^2 < r^2.  A line that misses the sphere
    // gets the mirrored (empty) interval, so that t_out - t_in measures the distance from the silhouette on both sides
    const float A = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float bA = (m[0] * d[0] + m[1] * d[1] + m[2] * d[2]) / A;
    const float q0 = m[0] - bA * d[0], q1 = m[1] - bA * d[1], q2 = m[2] - bA * d[2];
    const float e = c.radius * c.radius - (q0 * q0 + q1 * q1 + q2 * q2);
    const float h0 = sqrtf(fabsf(e) / A);
    const float h = e > 0.f ? h0 : -h0;
    t_in = -bA - h;
    t_out = -bA + h;
    if (WANT_N) { n[0] = m[0] + t_in * d[0]; n[1] = m[1] + t_in * d[1]; n[2] = m[2] + t_in * d[2]; }
  } else {
    t_in = -NM_RAY_INF;
    t_out = NM_RAY_INF;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float q = c.rot[a] * m[0] + c.rot[3 + a] * m[1] + c.rot[6 + a] * m[2];
      const float dq = c.rot[a] * d[0] + c.rot[3 + a] * d[1] + c.rot[6 + a] * d[2];
      float t0, t1;
      ray_slab(q, dq, -c.half[a], c.half[a], t0, t1);
      if (t0 > t_in) {
        t_in = t0;
        which = a;
        if (WANT_N) {
          const float sg = dq > 0.f ? -1.f : 1.f;
          n[0] = sg * c.rot[a]; n[1] = sg * c.rot[3 + a]; n[2] = sg * c.rot[6 + a];
        }
      }
      t_out = fminf(t_out, t1);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t0 = cube.t0[a], t1 = cube.t1[a];
    if (t0 > t_in) {
      t_in = t0;
      which = 3 + a;
      if (WANT_N) {
        const float sg = d[a] > 0.f ? -1.f : 1.f;
        n[0] = a == 0 ? sg : 0.f; n[1] = a == 1 ? sg : 0.f; n[2] = a == 2 ? sg : 0.f;
      }
    }
    t_out = fminf(t_out, t1);
  }
}
