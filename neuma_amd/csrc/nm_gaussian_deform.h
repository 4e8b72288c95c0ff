// The 3DGS parametrisation of one deformed Gaussian (nm_export.hip): (log-scales, raw quaternion, F) -> (log-scales', quaternion')
// with  build_rotation(q') diag(exp(ls'))^2 build_rotation(q')^T == F L L^T F^T,  L = build_rotation(normalize(q)) diag(mod exp(ls)).
// M = F L = U diag(s) V^T by nm_svd3 (U in SO(3) by construction, also for det F < 0), so F L L^T F^T = U diag(s^2) U^T: the scales
// are |s_i| and the rotation is U.  cov' itself is never formed: its eigen-decomposition would square the condition number.
// __host__ __device__, as nm_svd3 is: tests/export_host/ runs it without a GPU.
#pragma once
#include "nm_common.h"
#include "nm_gaussian.h"

namespace {

// rotation matrix (row-major, in SO(3) up to rounding) -> unit quaternion (r, x, y, z) with r >= 0.  Shepperd's branch on the largest
// of (trace, m00, m11, m22): each branch is 4 c (r, x, y, z) with c the component that branch makes largest (4 c^2 >= 1), so the
// common factor leaves with the normalisation and nothing small is ever divided by.
NM_HD void nm_rot_to_quat(const M3& R, float q[4]) {
  const float m00 = R.m[0], m11 = R.m[4], m22 = R.m[8], t = m00 + m11 + m22;
  float v[4];
  if (t >= m00 && t >= m11 && t >= m22) {
    v[0] = 1.f + t;           v[1] = R.m[7] - R.m[5];         v[2] = R.m[2] - R.m[6];         v[3] = R.m[3] - R.m[1];
  } else if (m00 >= m11 && m00 >= m22) {
    v[0] = R.m[7] - R.m[5];   v[1] = 1.f + m00 - m11 - m22;   v[2] = R.m[1] + R.m[3];         v[3] = R.m[2] + R.m[6];
  } else if (m11 >= m22) {
    v[0] = R.m[2] - R.m[6];   v[1] = R.m[1] + R.m[3];         v[2] = 1.f - m00 + m11 - m22;   v[3] = R.m[5] + R.m[7];
  } else {
    v[0] = R.m[3] - R.m[1];   v[1] = R.m[2] + R.m[6];         v[2] = R.m[5] + R.m[7];         v[3] = 1.f - m00 - m11 + m22;
  }
  const float inv = (v[0] < 0.f ? -1.f : 1.f) / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
#pragma unroll
  for (int a = 0; a < 4; ++a) q[a] = v[a] * inv;
}

// F: 9 floats row-major, or nullptr for the identity (which goes through the same product, so it is bitwise the explicit identity).
// Scales are clamped from below at max(1e-20 s_0, 1e-37) before the logarithm: a crushed axis (rank loss, F = 0) keeps a finite
// log-scale at least 20 decades under the largest one, and 1e-37 (what a scale becomes where s_0 itself is zero or below it) squares
// to zero in fp32 like the exact answer does.
NM_HD void nm_gaussian_deform_one(const float ls[3], const float rot[4], const float* F, float mod, float ls_out[3], float q_out[4]) {
  float e[3], q[4];
#pragma unroll
  for (int a = 0; a < 3; ++a) e[a] = mod * expf(ls[a]);
  qnormalize(rot, q);
  M3 Lm;
  quat_rot(q, Lm.m);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Lm.m[3 * a + b] *= e[b];
  const M3 M = m3_mul(F ? m3_load(F) : m3_ident(), Lm);
  M3 U, V;
  float s[3];
  nm_svd3(M, U, s, V);
  const float floor_s = fmaxf(1e-20f * s[0], 1e-37f);
#pragma unroll
  for (int a = 0; a < 3; ++a) ls_out[a] = logf(fmaxf(fabsf(s[a]), floor_s));
  nm_rot_to_quat(U, q_out);
}

}  // namespace
