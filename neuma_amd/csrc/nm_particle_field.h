// Field paint, the per-particle half (nm_paint.hip): one quantity of one particle, and one value through a colour map.  The
// definitions are in include/neuma_hip.h ("field paint") and, in fp64, in neuma_amd/extras/field_paint.py.
// __host__ __device__, as nm_svd3 is: tests/field_paint_host/ runs both functions without a GPU.
// The quantity is a template parameter: each instantiation names only the arrays it reads, so the others never become
// registers (or loads) of its kernel.
#pragma once
#include "nm_common.h"

namespace {

// 0 when every entry is finite, NaN otherwise (0 * Inf and 0 * NaN are NaN): added to a result that a non-finite input could
// otherwise leave finite (fmaxf drops a NaN, x / Inf is 0)
template <int N>
NM_HD float nm_field_poison(const float (&a)[N]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s += 0.f * a[i];
  return s;
}

NM_HD float nm_field_nan() { return nm_bits_to_float(0x7fc00000u); }

// x, v, x0: 3 floats; F, tau: row-major.  An argument quantity Q does not read is not touched (may be left uninitialised).
template <int Q>
NM_HD float nm_particle_field_one(const float* x, const float* v, const M3& F, const M3& tau, const float* x0) {
  if constexpr (Q == NM_FIELD_SPEED) return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if constexpr (Q == NM_FIELD_DISPLACEMENT) {
    const float d0 = x[0] - x0[0], d1 = x[1] - x0[1], d2 = x[2] - x0[2];
    return sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  }
  if constexpr (Q == NM_FIELD_VOLUME) return m3_det(F) + nm_field_poison(F.m);
  if constexpr (Q == NM_FIELD_STRAIN) {
    M3 U, V;
    float s[3], e[3];
    nm_svd3(F, U, s, V);
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = logf(fmaxf(fabsf(s[a]), 1e-20f));
    const float m = (e[0] + e[1] + e[2]) * (1.f / 3.f);
    const float d0 = e[0] - m, d1 = e[1] - m, d2 = e[2] - m;
    return sqrtf((2.f / 3.f) * (d0 * d0 + d1 * d1 + d2 * d2)) + nm_field_poison(F.m);
  }
  // the two stress quantities: Cauchy stress tau / J, undefined for an inverted particle
  const float J = m3_det(F);
  const float bad = nm_field_poison(F.m) + nm_field_poison(tau.m);
  const float tr = tau.m[0] + tau.m[4] + tau.m[8];
  if constexpr (Q == NM_FIELD_PRESSURE) return J > 0.f ? -tr / (3.f * J) + bad : nm_field_nan();
  // von Mises: the deviator of the symmetrised tau, scaled by 1 / J at the end (sqrt(3/2) |dev sym tau| / J)
  const float mean = tr * (1.f / 3.f);
  const float a0 = tau.m[0] - mean, a1 = tau.m[4] - mean, a2 = tau.m[8] - mean;
  const float o01 = 0.5f * (tau.m[1] + tau.m[3]), o02 = 0.5f * (tau.m[2] + tau.m[6]), o12 = 0.5f * (tau.m[5] + tau.m[7]);
  const float ss = a0 * a0 + a1 * a1 + a2 * a2 + 2.f * (o01 * o01 + o02 * o02 + o12 * o12);
  return J > 0.f ? sqrtf(1.5f * ss) / J + bad : nm_field_nan();
}

// a colour map by value: it travels in the kernel arguments, and the knots are picked by selects over a loop that is unrolled
// (an index chosen per lane would move the table into scratch memory)
struct NmPaintMap {
  int n;
  float c[NM_PAINT_MAX_KNOTS][3];
  float nodata[3];
};

// g through the map over [lo, hi] -> the SH DC coefficients of its colour
NM_HD void nm_field_color(float g, float lo, float hi, const NmPaintMap& map, float dc[3]) {
  const float w = hi - lo;
  float t = (g - lo) / w;
  const float big = 3.402823466e+38f;
  const bool ok = fabsf(g) <= big && fabsf(lo) <= big && w > 0.f && w <= big;
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float tn = t * (float)(map.n - 1);
  const int fl = (int)floorf(tn);
  const int i = fl < map.n - 2 ? fl : map.n - 2;
  const float u = tn - (float)i;
  float rgb[3] = {map.nodata[0], map.nodata[1], map.nodata[2]};
#pragma unroll
  for (int k = 0; k < NM_PAINT_MAX_KNOTS - 1; ++k) {
    if (k < map.n - 1) {
      const bool here = ok && i == k;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[ch] = here ? map.c[k][ch] + u * (map.c[k + 1][ch] - map.c[k][ch]) : rgb[ch];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) dc[ch] = (rgb[ch] - 0.5f) / 0.28209479177387814f;
}

}  // namespace
