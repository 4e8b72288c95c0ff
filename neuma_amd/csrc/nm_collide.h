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

// ---- the same two functions with the collider's pose and its own velocity at the node as ARGUMENTS: collide_normal(c, p, n) is
// collide_normal(c, c.center, c.rot, p, n) and collide_apply(c, p, u) is collide_apply(c, c.center, c.rot, p, c.velocity, u).  They
// are spelled twice on purpose: routed through these, the kernels of a handle without rigid bodies came out of the compiler with
// another choice of fused multiply-adds (k_grid_collide: two subtractions of vt = w - vn n contracted), i.e. with other last bits,
// and a handle without bodies has to compute what it computed.  Forward only: bodies have no adjoint.
__device__ __forceinline__ bool collide_normal(const nm_collider& c, const float center[3], const float rot[9], const float p[3],
                                               float n[3]) {
  const float d[3] = {p[0] - center[0], p[1] - center[1], p[2] - center[2]};
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
    q[a] = rot[a] * d[0] + rot[3 + a] * d[1] + rot[6 + a] * d[2];
    pen[a] = c.half[a] - fabsf(q[a]);
  }
  if (!(pen[0] > 0.f && pen[1] > 0.f && pen[2] > 0.f)) return false;
  int best = 0;
  if (pen[1] < pen[best]) best = 1;
  if (pen[2] < pen[best]) best = 2;
  const float sgn = sel3(q, best) < 0.f ? -1.f : 1.f;
  n[0] = sgn * (best == 0 ? rot[0] : (best == 1 ? rot[1] : rot[2]));
  n[1] = sgn * (best == 0 ? rot[3] : (best == 1 ? rot[4] : rot[5]));
  n[2] = sgn * (best == 0 ? rot[6] : (best == 1 ? rot[7] : rot[8]));
  return true;
}

// vc: the collider's own velocity AT THIS NODE (a rigid body: v + w x (p - c), rigid_velocity below)
__device__ __forceinline__ bool collide_apply(const nm_collider& c, const float center[3], const float rot[9], const float p[3],
                                              const float vc[3], float u[3]) {
  float n[3];
  if (!collide_normal(c, center, rot, p, n)) return false;
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

// ---- rigid bodies (include/neuma_hip.h "Rigid bodies"): a sphere or box entry whose pose and velocity field come from a small
// device record instead of the by-value set.  k_rigid_step (nm_rigid.h) refreshes the record once per substep; it is indexed by
// the collider's place in the set and wave-uniform, so a wave reads it through scalar loads like the set itself.
struct RigidPose {
  float c[3];      // centre
  float R[9];      // R(q), row-major like nm_collider.rot
  float v[3];      // P / M
  float w[3];      // omega, simulation axes
};
struct RigidView {
  unsigned mask;                           // bit c: entry c of the set is a body
  const RigidPose* __restrict__ pose;      // [NM_MAX_COLLIDERS], valid where the mask says so
};

// v_c(p) = v + w x (p - c): three fp32 roundings per component on top of the prescribed collider's constant
__device__ __forceinline__ void rigid_velocity(const RigidPose& b, const float p[3], float vc[3]) {
  const float d[3] = {p[0] - b.c[0], p[1] - b.c[1], p[2] - b.c[2]};
  vc[0] = b.v[0] + (b.w[1] * d[2] - b.w[2] * d[1]);
  vc[1] = b.v[1] + (b.w[2] * d[0] - b.w[0] * d[2]);
  vc[2] = b.v[2] + (b.w[0] * d[1] - b.w[1] * d[0]);
}
// entry c of the set applied at p, wherever its pose lives.  BODIES = false is collide_apply(S.c[c], p, u) and nothing else: the
// kernels of a handle without bodies are the instantiations that never look at the view.
template <bool BODIES>
__device__ __forceinline__ bool collide_apply_entry(const ColliderSet& S, const RigidView& B, int c, const float p[3], float u[3]) {
  if (BODIES && ((B.mask >> c) & 1u)) {
    const RigidPose b = B.pose[c];      // (by value: wave-uniform, so the whole record comes through scalar loads)
    float vc[3];
    rigid_velocity(b, p, vc);
    return collide_apply(S.c[c], b.c, b.R, p, vc, u);
  }
  return collide_apply(S.c[c], p, u);
}
template <bool BODIES>
__device__ __forceinline__ bool collide_normal_entry(const ColliderSet& S, const RigidView& B, int c, const float p[3], float n[3]) {
  if (BODIES && ((B.mask >> c) & 1u)) {
    const RigidPose b = B.pose[c];
    return collide_normal(S.c[c], b.c, b.R, p, n);
  }
  return collide_normal(S.c[c], p, n);
}
