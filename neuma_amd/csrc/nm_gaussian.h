// Per-Gaussian device functions of the chain (log-scales, quaternion) -> cov6 and its adjoint (general_utils.py:93-139),
// shared by the registration kernels (nm_regist.hip) and the activation kernels (nm_gauss.hip).
#pragma once

namespace {

// F.normalize (eps 1e-12); returns the divisor.  (This and quat_rot also run on the host: nm_gaussian_deform.h.)
__host__ __device__ __forceinline__ float qnormalize(const float* v, float* n) {
  const float len = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]), 1e-12f);
#pragma unroll
  for (int i = 0; i < 4; ++i) n[i] = v[i] / len;
  return len;
}

// build_rotation (general_utils.py:101-124) of an already normalised quaternion
__host__ __device__ __forceinline__ void quat_rot(const float* q, float* M) {
  const float r = q[0], x = q[1], y = q[2], z = q[3];
  M[0] = 1.f - 2.f * (y * y + z * z); M[1] = 2.f * (x * y - r * z);       M[2] = 2.f * (x * z + r * y);
  M[3] = 2.f * (x * y + r * z);       M[4] = 1.f - 2.f * (x * x + z * z); M[5] = 2.f * (y * z - r * x);
  M[6] = 2.f * (x * z - r * y);       M[7] = 2.f * (y * z + r * x);       M[8] = 1.f - 2.f * (x * x + y * y);
}

// its adjoint w.r.t. q = (r, x, y, z)
__device__ __forceinline__ void quat_rot_adj(const float* q, const float* dM, float* dq) {
  const float r = q[0], x = q[1], y = q[2], z = q[3];
  dq[0] = 2.f * (-z * dM[1] + y * dM[2] + z * dM[3] - x * dM[5] - y * dM[6] + x * dM[7]);
  dq[1] = 2.f * (y * dM[1] + z * dM[2] + y * dM[3] - 2.f * x * dM[4] - r * dM[5] + z * dM[6] + r * dM[7] - 2.f * x * dM[8]);
  dq[2] = 2.f * (-2.f * y * dM[0] + x * dM[1] + r * dM[2] + x * dM[3] + z * dM[5] - r * dM[6] + z * dM[7] - 2.f * y * dM[8]);
  dq[3] = 2.f * (-2.f * z * dM[0] - r * dM[1] + x * dM[2] + r * dM[3] - 2.f * z * dM[4] + y * dM[5] + x * dM[6] + y * dM[7]);
}

// d(v / |v|) adjoint: dv = (dn - n (n . dn)) / |v|
__device__ __forceinline__ void norm_adj(const float* n, float len, const float* dn, float* dv) {
  const float p = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2] + n[3] * dn[3];
#pragma unroll
  for (int a = 0; a < 4; ++a) dv[a] = (dn[a] - n[a] * p) / len;
}

// cov6[6 i .. 6 i + 5] = strip_symmetric(L L^T), L = M diag(e)
__device__ __forceinline__ void cov6_build(const float* M, const float* e, float* __restrict__ cov6, int i) {
  float Lm[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Lm[3 * a + b] = M[3 * a + b] * e[b];
  const int idx[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int a = idx[c][0], b = idx[c][1];
    cov6[6 * i + c] = Lm[3 * a] * Lm[3 * b] + Lm[3 * a + 1] * Lm[3 * b + 1] + Lm[3 * a + 2] * Lm[3 * b + 2];
  }
}

// its adjoint: dL = (G + G^T) L with G holding the six upstream values g6 in the upper triangle; dM = dL diag(e), and for
// every axis b the caller's on_de(b, de_b) with de_b = sum_a dL[a][b] M[a][b]
template <class OnDe>
__device__ __forceinline__ void cov6_adj(const float* g6, const float* M, const float* e, float* dM, OnDe on_de) {
  const float S[9] = {2.f * g6[0], g6[1], g6[2], g6[1], 2.f * g6[3], g6[4], g6[2], g6[4], 2.f * g6[5]};
  float Lm[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Lm[3 * a + b] = M[3 * a + b] * e[b];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    float de = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float dLab = S[3 * a] * Lm[b] + S[3 * a + 1] * Lm[3 + b] + S[3 * a + 2] * Lm[6 + b];
      dM[3 * a + b] = dLab * e[b];
      de += dLab * M[3 * a + b];
    }
    on_de(b, de);
  }
}

}  // namespace
