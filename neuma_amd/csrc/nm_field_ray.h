// Ray / segment versus the DRAWN SOLID of a field collider: a sphere trace of the trilinearly interpolated phi (definition:
// include/neuma_hip.h "Drawing mesh colliders", fp64 yardstick: neuma_amd/extras/mesh_draw.py, which spells the same operations
// in the same order).  The drawn solid is {phi < 0} cut by the lattice box [origin, origin + (dims - 1) spacing] and by the unit
// cube.  field_trace is the one trace both kernels of nm_draw.hip use: k_field_cast per pixel (WANT_N: polished t and the normal),
// k_field_hide per Gaussian (the decision only).
//   interval  [t0, t1] = t >= 0, the cube's three slabs, the lattice's three slabs; t_end = min(t1, t_cap)
//   which     -1: t0 = 0 (the origin is inside both boxes); 0..2 the cube's axis, 3..5 the lattice's axis that gave t0 (strict >:
//             of equal entries the first stays); 6: the surface, found by the march
//   face hit  phi(t0) < 0: the hit is at t0 with that slab's normal
//   march     at most NM_FIELD_STEPS times: phi <= tau = 1e-3 spacing -> converged; else t += max(phi, tau) / L, and a miss once
//             t >= t_end.  L = |d|: phi is a distance in simulation units, t the parameter of o + t d
//   polish    three Newton steps t -= phi / (grad . d), each taken only while grad . d < 0, t kept inside [t0, t1]
// d need not be a unit vector.  The eight phi loads of a sample are the only memory traffic; the cell index is clamped to
// 0 .. dims - 2 on both sides (a point a rounding error outside the lattice extrapolates its border cell; NaN and inf land in a
// valid cell too), so every load lies inside the prod(dims) floats of phi.  No arrays indexed at run time.
#pragma once
#include "nm_collide_field.h"
#include "nm_collide_ray.h"

#define NM_FIELD_STEPS 192

// phi at o + t d [and with WANT_G the gradient of the interpolant per cell: divide by spacing for simulation units]
template <bool WANT_G>
__device__ __forceinline__ float field_sample(const nm_field_collider& c, const float o[3], const float d[3], float t, float g[3]) {
  float fr[3];
  int i[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = o[a] + t * d[a];
    const float q = (p - c.origin[a]) / c.spacing;
    const float f = fmaxf(fminf(floorf(q), (float)(c.dims[a] - 2)), 0.f);
    i[a] = (int)f;
    fr[a] = q - f;
  }
  const size_t sy = (size_t)c.dims[2], sx = (size_t)c.dims[1] * sy;
  const FieldCell k = field_cell(c.phi + ((size_t)i[0] * sx + (size_t)i[1] * sy + (size_t)i[2]), sx, sy, fr);
  if (WANT_G) {
    g[0] = k.gx;
    field_cell_grad_yz(k, fr, g[1], g[2]);
  }
  return k.phi;
}

// Does the ray o + t d, 0 <= t < t_cap, hit the drawn solid of c?  t_hit: where; with WANT_N `which` (above) and n, the outward
// normal in simulation coordinates (a face's axis, or grad / |grad|, +x where the gradient vanishes).
template <bool WANT_N>
__device__ __forceinline__ bool field_trace(const nm_field_collider& c, const float o[3], const float d[3], float L, const RayCube& cube,
                                            float t_cap, float& t_hit, int& which, float n[3]) {
  float t0 = 0.f, t1 = NM_RAY_INF;
  which = -1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (cube.t0[a] > t0) { t0 = cube.t0[a]; which = a; }
    t1 = fminf(t1, cube.t1[a]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float s0, s1;
    ray_slab(o[a], d[a], c.origin[a], c.origin[a] + (float)(c.dims[a] - 1) * c.spacing, s0, s1);
    if (s0 > t0) { t0 = s0; which = 3 + a; }
    t1 = fminf(t1, s1);
  }
  const float t_end = fminf(t1, t_cap);
  if (!(t0 < t_end)) return false;
  const float tau = 1e-3f * c.spacing;
  float g[3];
  float phi = field_sample<false>(c, o, d, t0, g);
  if (phi < 0.f) {
    t_hit = t0;
    if (WANT_N) {
      const int ax = which < 3 ? which : which - 3;
      const float dq = ax == 0 ? d[0] : (ax == 1 ? d[1] : d[2]);
      const float sg = dq > 0.f ? -1.f : 1.f;
      n[0] = ax == 0 ? sg : 0.f; n[1] = ax == 1 ? sg : 0.f; n[2] = ax == 2 ? sg : 0.f;
    }
    return true;
  }
  float t = t0;
  bool conv = false;
  for (int it = 0; it < NM_FIELD_STEPS; ++it) {
    if (phi <= tau) { conv = true; break; }
    t += fmaxf(phi, tau) / L;
    if (t >= t_end) break;
    phi = field_sample<false>(c, o, d, t, g);
  }
  if (!conv) return false;
  if (WANT_N) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      phi = field_sample<true>(c, o, d, t, g);
      const float gd = (g[0] / c.spacing) * d[0] + (g[1] / c.spacing) * d[1] + (g[2] / c.spacing) * d[2];
      if (gd < 0.f) t = fminf(fmaxf(t - phi / gd, t0), t1);
    }
    field_sample<true>(c, o, d, t, g);
    const float l2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    if (l2 > 0.f) {
      const float len = sqrtf(l2);
      n[0] = g[0] / len; n[1] = g[1] / len; n[2] = g[2] / len;
    } else {
      n[0] = 1.f; n[1] = 0.f; n[2] = 0.f;
    }
    which = 6;
  }
  t_hit = t;
  return true;
}
