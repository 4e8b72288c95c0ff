// Contact report of the per-operator MPM path (no reference counterpart; definition: include/neuma_hip.h "Contact report", fp64
// yardstick: neuma_amd/extras/contact.py).  contact_node adds one grid node's terms of one row - row 0 the box walls, row r the
// r-th obstacle of the chain, analytic colliders first - to nine fp64 accumulators.  The velocities are those of the substep:
// grid_velocity, then collide_apply / field_apply replayed in fp32 up to the row's obstacle, exactly as the forward kernels apply
// them; only the differences, their products with the mass and the lever arm, and the sums are fp64.  The kernels that sweep the
// active blocks with it (k_contact_rows, k_contact_sum) and their launch site are in nm_mpm.hip.
#pragma once
#include "nm_common.h"
#include "nm_grid.h"
#include "nm_collide.h"
#include "nm_collide_field.h"

// columns of a row: J[3], L[3], N, mass, nodes (NM_CONTACT_COLS of neuma_hip.h)
#define NM_CONTACT_N NM_CONTACT_COLS

// a: the node's {mv, m}; row is wave-uniform.  Nodes without mass carry no momentum and add nothing.  BODIES: entries of A that the
// view B marks take pose and velocity field from its record (nm_collide.h); false never looks at B.
template <bool BODIES>
__device__ __forceinline__ void contact_node(const MpmK& K, const ColliderSet& A, const RigidView& B, const FieldColliderSet& F, int row,
                                             int i, int j, int k, const float4& a, double acc[NM_CONTACT_N]) {
  if (!(a.w > 0.f)) return;
  float u[3], mk[3];
  grid_velocity(K, i, j, k, a, u, mk);
  float un[3] = {u[0] * mk[0], u[1] * mk[1], u[2] * mk[2]};      // u^(1), as k_grid_op stores it
  float n[3] = {0.f, 0.f, 0.f};
  bool inside;
  if (row == 0) {      // the walls: u^(0) -> u^(1); "inside" is the boundary layer, the only place the mask can be 0
    const int hi = K.G - K.bound;
    inside = i < K.bound || j < K.bound || k < K.bound || i >= hi || j >= hi || k >= hi;
  } else {
    const float p[3] = {(float)i * K.dx, (float)j * K.dx, (float)k * K.dx};
    const int c = row - 1;
    u[0] = un[0]; u[1] = un[1]; u[2] = un[2];
    const int na = c < A.n ? c : A.n;
    for (int e = 0; e < na; ++e) collide_apply_entry<BODIES>(A, B, e, p, u);
    if (c < A.n) {
      un[0] = u[0]; un[1] = u[1]; un[2] = u[2];
      inside = collide_apply_entry<BODIES>(A, B, c, p, un);
      if (inside) collide_normal_entry<BODIES>(A, B, c, p, n);
    } else {
      const int f = c - A.n;
      for (int e = 0; e < f; ++e) field_apply(F.c[e], p, u);
      un[0] = u[0]; un[1] = u[1]; un[2] = u[2];
      inside = field_apply(F.c[f], p, un);
      if (inside) field_normal(F.c[f], p, n);
    }
  }
  if (!inside) return;
  const double m = (double)a.w;
  const double inv_g = 1.0 / (double)K.G;
  const double p[3] = {(double)i * inv_g, (double)j * inv_g, (double)k * inv_g};
  const double d[3] = {(double)u[0] - (double)un[0], (double)u[1] - (double)un[1], (double)u[2] - (double)un[2]};      // u^(r) - u^(r+1)
  acc[0] += m * d[0];
  acc[1] += m * d[1];
  acc[2] += m * d[2];
  acc[3] += m * (p[1] * d[2] - p[2] * d[1]);
  acc[4] += m * (p[2] * d[0] - p[0] * d[2]);
  acc[5] += m * (p[0] * d[1] - p[1] * d[0]);
  acc[6] -= m * (d[0] * (double)n[0] + d[1] * (double)n[1] + d[2] * (double)n[2]);
  acc[7] += m;
  acc[8] += 1.0;
}
