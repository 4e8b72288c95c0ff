// Field colliders of the per-operator MPM path: obstacles whose shape is a signed distance field on a regular lattice (a mesh:
// neuma_amd/mesh_sdf.py).  No reference counterpart; definition: include/neuma_hip.h "Field colliders", fp64 yardstick:
// neuma_amd/extras/colliders.py apply_field_collider.  field_cell is the trilinear sample, field_normal the geometry (phi and
// its analytic gradient in the cell that holds the node), field_apply one collider's response at one node, field_adjoint the transpose of its Jacobian
// du'/du.  The response given the normal is the sticky / slip / friction law of nm_collide.h, spelled again here: nm_collide.h
// and the kernels built from it stay as they are.  The kernels that sweep the active blocks (k_grid_collide_field,
// k_grid_collide_field_bwd) and their launch sites are in nm_mpm.hip; the set travels by value in the kernel arguments, and
// the eight phi loads of a node inside a lattice are the only memory traffic.
#pragma once
#include "nm_common.h"

struct FieldColliderSet {
  int n;
  nm_field_collider c[NM_MAX_FIELD_COLLIDERS];
};

// The trilinear interpolant of one lattice cell, in two steps so that a caller that only needs the sign pays for no more: the
// eight corner values at f (strides sx, sy, 1) and the fractions t give phi and g_x (field_cell); the same intermediate values
// give g_y and g_z (field_cell_grad_yz).  The gradient is that of the interpolant in t: per cell, not per unit length.
// Shared by field_normal (the grid) and the sphere trace of nm_field_ray.h (the renders).
struct FieldCell {
  float d00, d01, d10, d11;      // the z differences, whose bilinear interpolant is d phi / d t_z
  float e0, e1;                  // y differences at x0, x1
  float gx, phi;
};
__device__ __forceinline__ FieldCell field_cell(const float* __restrict__ f, size_t sx, size_t sy, const float t[3]) {
  const float f000 = f[0], f001 = f[1], f010 = f[sy], f011 = f[sy + 1];
  const float f100 = f[sx], f101 = f[sx + 1], f110 = f[sx + sy], f111 = f[sx + sy + 1];
  FieldCell k;
  // along z, then y, then x
  k.d00 = f001 - f000; k.d01 = f011 - f010; k.d10 = f101 - f100; k.d11 = f111 - f110;
  const float a00 = f000 + t[2] * k.d00, a01 = f010 + t[2] * k.d01, a10 = f100 + t[2] * k.d10, a11 = f110 + t[2] * k.d11;
  k.e0 = a01 - a00; k.e1 = a11 - a10;
  const float b0 = a00 + t[1] * k.e0, b1 = a10 + t[1] * k.e1;
  k.gx = b1 - b0;
  k.phi = b0 + t[0] * k.gx;
  return k;
}
__device__ __forceinline__ void field_cell_grad_yz(const FieldCell& k, const float t[3], float& gy, float& gz) {
  gy = k.e0 + t[0] * (k.e1 - k.e0);
  const float z0 = k.d00 + t[1] * (k.d01 - k.d00), z1 = k.d10 + t[1] * (k.d11 - k.d10);
  gz = z0 + t[0] * (z1 - z0);
}

// is the node at p inside the field collider (phi < 0)?  n: the outward unit normal there (only defined when inside).
// A node off the lattice - or a NaN coordinate - is outside.  The cell index is clamped to dims - 2, so the eight corners read
// always lie inside the prod(dims) floats of phi.
__device__ __forceinline__ bool field_normal(const nm_field_collider& c, const float p[3], float n[3]) {
  float t[3];
  int i[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = (p[a] - c.origin[a]) / c.spacing;
    if (!(q >= 0.f && q <= (float)(c.dims[a] - 1))) return false;
    const float f = fminf(floorf(q), (float)(c.dims[a] - 2));
    i[a] = (int)f;
    t[a] = q - f;
  }
  const size_t sy = (size_t)c.dims[2], sx = (size_t)c.dims[1] * sy;
  const FieldCell k = field_cell(c.phi + ((size_t)i[0] * sx + (size_t)i[1] * sy + (size_t)i[2]), sx, sy, t);
  if (!(k.phi < 0.f)) return false;
  const float gx = k.gx;
  float gy, gz;
  field_cell_grad_yz(k, t, gy, gz);
  const float l2 = gx * gx + gy * gy + gz * gz;
  if (l2 > 0.f) {
    const float inv = 1.f / sqrtf(l2);
    n[0] = gx * inv; n[1] = gy * inv; n[2] = gz * inv;
  } else {
    n[0] = 1.f; n[1] = 0.f; n[2] = 0.f;
  }
  return true;
}

// u -> u' at the node at p; returns whether the node lies inside the collider (u is untouched otherwise)
__device__ __forceinline__ bool field_apply(const nm_field_collider& c, const float p[3], float u[3]) {
  float n[3];
  if (!field_normal(c, p, n)) return false;
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

// g = dL/du' -> dL/du, with u the velocity field_apply was given at this node (the formulas of collide_adjoint, nm_collide.h)
__device__ __forceinline__ bool field_adjoint(const nm_field_collider& c, const float p[3], const float u[3], float g[3]) {
  float n[3];
  if (!field_normal(c, p, n)) return false;
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
