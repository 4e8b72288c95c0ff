// Colliders of the per-operator MPM path (no reference counterpart; definition: include/neuma_hip.h, fp64 yardstick:
// neuma_amd/extras/colliders.py).  Rigid half-spaces, spheres and oriented boxes that rewrite the node velocities behind the
// box boundary condition of grid_velocity (nm_grid.h): collide_apply is one collider's response at one node, collide_adjoint
// the transpose of its Jacobian du'/du.  The kernels that sweep the active blocks with them (k_grid_collide,
// k_grid_collide_bwd) and their launch sites are in nm_mpm.hip; the set travels by value in the kernel arguments, so a wave
// reads it through scalar loads and no lane holds a copy.
#pragma once
#include "nm_common.h"
#include "nm_grid.h"

struct ColliderSet {
  int n;
  nm_collider c[NM_MAX_COLLIDERS];
};

// is the point p inside collider c (sdf < 0)?  n: the outward unit normal there (only defined when inside)
__device__ __forceinline__ bool collide_normal(const nm_collider& c, const float p[3], float n[3]) {
  const float d[3] = {p[0] - c.center[0], p[1] - c.center[1], p[2] - c.center[2]};
  if (c.shape == NM_COLLIDER_PLANE) {
    n[0] = c.normal[0]; n[1] = c.normal[1]; n[2] = c.normal[2];
    return d[0] * n[0] + d[1] * n[1] + d[2] * n[2] < 0.f;
  }
  if (c.shape == NM_COLLIDER_SPHERE) {
    const float r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(r2 < c.radius * c.radius)) return false;
    if (r2 > 0.f) {
      const float inv = 1.f / sqrtf(r2);
      n[0] = d[0] * inv; n[1] = d[1] * inv; n[2] = d[2] * inv;
    } else {
      n[0] = 1.f; n[1] = 0.f; n[2] = 0.f;
    }
    return true;
  }
  // oriented box: q = R^T d are the box's own coordinates; the face with the smallest penetration depth gives the normal
  // (strict <: a tie keeps the lowest axis)
  float q[3], pen[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q[a] = c.rot[a] * d[0] + c.rot[3 + a] * d[1] + c.rot[6 + a] * d[2];
    pen[a] = c.half[a] - fabsf(q[a]);
  }
  if (!(pen[0] > 0.f && pen[1] > 0.f && pen[2] > 0.f)) return false;
  int best = 0;
  if (pen[1] < pen[best]) best = 1;
  if (pen[2] < pen[best]) best = 2;
  const float sgn = sel3(q, best) < 0.f ? -1.f : 1.f;
  n[0] = sgn * (best == 0 ? c.rot[0] : (best == 1 ? c.rot[1] : c.rot[2]));
  n[1] = sgn * (best == 0 ? c.rot[3] : (best == 1 ? c.rot[4] : c.rot[5]));
  n[2] = sgn * (best == 0 ? c.rot[6] : (best == 1 ? c.rot[7] : c.rot[8]));
  return true;
}

// u -> u' at the node at p; returns whether the node lies inside the collider (u is untouched otherwise)
__device__ __forceinline__ bool collide_apply(const nm_collider& c, const float p[3], float u[3]) {
  float n[3];
  if (!collide_normal(c, p, n)) return false;
  const float* vc = c.velocity;
  if (c.surface == NM_SURFACE_STICKY) {
    u[0] = vc[0]; u[1] = vc[1]; u[2] = vc[2];
    return true;
  }
  const float w[3] = {u[0] - vc[0], u[1] - vc[1], u[2] - vc[2]};
  const float vn = w[0] * n[0] + w[1] * n[1] + w[2] * n[2];
  if (!(vn < 0.f)) return true;      // separating: kept
  if (c.surface == NM_SURFACE_SLIP) {
    u[0] -= vn * n[0]; u[1] -= vn * n[1]; u[2] -= vn * n[2];
    return true;
  }
  const float vt[3] = {w[0] - vn * n[0], w[1] - vn * n[1], w[2] - vn * n[2]};
  const float s = sqrtf(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
  const float f = s > 0.f ? fmaxf(0.f, 1.f + c.friction * vn / s) : 0.f;
  u[0] = vc[0] + f * vt[0]; u[1] = vc[1] + f * vt[1]; u[2] = vc[2] + f * vt[2];
  return true;
}

// g = dL/du' -> dL/du, with u the velocity collide_apply was given at this node
//   sticky: 0.  slip (vn < 0): P g, P = I - n n^T.  friction (vn < 0, s > 0, f > 0): f P g + mu (vt.g) (n / s - vn vt / s^3),
//   0 where the Coulomb cone clamps (f = 0) or vt = 0.  Separating or outside: g.
__device__ __forceinline__ bool collide_adjoint(const nm_collider& c, const float p[3], const float u[3], float g[3]) {
  float n[3];
  if (!collide_normal(c, p, n)) return false;
  if (c.surface == NM_SURFACE_STICKY) {
    g[0] = g[1] = g[2] = 0.f;
    return true;
  }
  const float* vc = c.velocity;
  const float w[3] = {u[0] - vc[0], u[1] - vc[1], u[2] - vc[2]};
  const float vn = w[0] * n[0] + w[1] * n[1] + w[2] * n[2];
  if (!(vn < 0.f)) return true;
  const float gn = g[0] * n[0] + g[1] * n[1] + g[2] * n[2];
  const float pg[3] = {g[0] - gn * n[0], g[1] - gn * n[1], g[2] - gn * n[2]};
  if (c.surface == NM_SURFACE_SLIP) {
    g[0] = pg[0]; g[1] = pg[1]; g[2] = pg[2];
    return true;
  }
  const float vt[3] = {w[0] - vn * n[0], w[1] - vn * n[1], w[2] - vn * n[2]};
  const float s = sqrtf(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
  const float f = s > 0.f ? 1.f + c.friction * vn / s : 0.f;
  if (!(f > 0.f)) {
    g[0] = g[1] = g[2] = 0.f;
    return true;
  }
  const float inv_s = 1.f / s;
  const float k = c.friction * (vt[0] * g[0] + vt[1] * g[1] + vt[2] * g[2]) * inv_s;      // mu (vt.g) / s
  const float kt = k * vn * inv_s * inv_s;
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = f * pg[a] + k * n[a] - kt * vt[a];
  return true;
}
