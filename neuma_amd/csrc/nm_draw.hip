// Drawing colliders in renders (no reference counterpart; definition: include/neuma_hip.h "Drawing colliders", fp64 yardstick:
// neuma_amd/extras/collider_draw.py).  Three kernels around unchanged nm_raster_forward_ex calls:
//   k_collider_cast     per pixel: nearest hit of the pixel's ray over the drawn solids -> t, shade, hit
//   k_collider_hide     per Gaussian: opacity 0 where the segment camera -> mean meets a drawn solid
//   k_collider_compose  per pixel: rgb_front + (1 - a_front) shade where hit, img_all elsewhere
// and, for mesh (field) colliders, two in-out passes behind the first two (definition: "Drawing mesh colliders"; the trace:
// csrc/nm_field_ray.h; fp64 yardstick: neuma_amd/extras/mesh_draw.py):
//   k_field_cast        per pixel: a sphere trace of each field's phi, merged into t, shade, hit where it is nearer
//   k_field_hide        per Gaussian: the same trace on the segment camera -> mean, merged into opacity_front / hidden
// The collider set, the styles, the ray basis and the affine map travel by value in the kernel arguments (as ColliderSet
// does in nm_mpm.hip): the loop over the colliders and the branch on the shape are wave-uniform and read through scalar
// loads.  No LDS, no atomics, no workspace.  Built with -ffp-contract=off (csrc/Makefile): the yardstick's fp32 evaluation
// spells the same operations in the same order, and the tests hold the kernels to 4x its distance from fp64.
#include <math.h>

#include "nm_collide_ray.h"
#include "nm_field_ray.h"

namespace {

constexpr int kDrawThreads = 256;      // 4 waves, each 64 consecutive pixels of one row / 64 consecutive Gaussians

struct DrawStyle {
  float color[3];
  float checker;      // cell size (simulation units) on a plane's own face; 0: plain
  float u[3], v[3];   // the plane's 2-D frame (host, fp64: plane_frame)
};

struct DrawSet {
  int n;
  nm_collider c[NM_MAX_COLLIDERS];
  float a[3];         // render = a * sim + b, per axis
  float o_s[3];       // the camera in simulation coordinates: (campos - b) / a
};

struct DrawStyles {
  DrawStyle s[NM_MAX_COLLIDERS];
};

struct RayBasis {     // direction of the ray through ndc (x, y): x gx + y gy + g0 (render coordinates, not normalised)
  float gx[3], gy[3], g0[3];
};

// one pixel: the nearest hit of its ray (t = +inf, hit = -1, rgb = 0 without one)
__device__ __forceinline__ void cast_pixel(int px, int py, int H, int W, const DrawSet& set, const DrawStyles& sty, const RayBasis& rb,
                                           float& best_t, int& best, float rgb[3]) {
  const float nx = (float)(2 * px + 1) / (float)W - 1.f, ny = (float)(2 * py + 1) / (float)H - 1.f;
  float dr[3], ds[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) dr[a] = nx * rb.gx[a] + ny * rb.gy[a] + rb.g0[a];
  const float len = sqrtf(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dr[a] = dr[a] / len;
    ds[a] = dr[a] / set.a[a];
  }
  const RayCube cube = ray_cube(set.o_s, ds);
  best_t = NM_RAY_INF;
  best = -1;
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  for (int i = 0; i < set.n; ++i) {
    const nm_collider& c = set.c[i];
    const DrawStyle& s = sty.s[i];
    float t_in, t_o, n[3];
    int which;
    ray_solid<true>(c, set.o_s, ds, cube, t_in, t_o, which, n);
    const bool is_hit = t_in < t_o && t_o > 0.f;
    const float t = fmaxf(t_in, 0.f);
    if (!(is_hit && t < best_t)) continue;
    best_t = t;
    best = i;
    // n_r = normalize(n_s / a); the headlight l = -d_r.  Camera inside the solid: the normal faces the camera, n.l = 1
    const float nr0 = n[0] / set.a[0], nr1 = n[1] / set.a[1], nr2 = n[2] / set.a[2];
    const float nl = sqrtf(nr0 * nr0 + nr1 * nr1 + nr2 * nr2);
    float ndl = -(nr0 * dr[0] + nr1 * dr[1] + nr2 * dr[2]) / nl;
    ndl = t_in < 0.f ? 1.f : ndl;
    float k = 1.f;
    if (c.shape == NM_COLLIDER_PLANE && s.checker > 0.f) {
      const float r0 = set.o_s[0] + t * ds[0] - c.center[0], r1 = set.o_s[1] + t * ds[1] - c.center[1],
                  r2 = set.o_s[2] + t * ds[2] - c.center[2];
      const float cu = (r0 * s.u[0] + r1 * s.u[1] + r2 * s.u[2]) / s.checker;
      const float cv = (r0 * s.v[0] + r1 * s.v[1] + r2 * s.v[2]) / s.checker;
      const bool odd = (((int)floorf(cu) + (int)floorf(cv)) & 1) != 0;
      k = (which == 0 && !(t_in < 0.f) && odd) ? 0.8f : 1.f;
    }
    const float lam = 0.35f + 0.65f * fmaxf(0.f, ndl);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = s.color[ch] * k * lam;
  }
}

// one Gaussian: does the segment camera -> mean (render coordinates) meet a drawn solid before the mean?
__device__ __forceinline__ bool hide_one(const DrawSet& set, float cx, float cy, float cz, float mx, float my, float mz) {
  const float ds[3] = {(mx - cx) / set.a[0], (my - cy) / set.a[1], (mz - cz) / set.a[2]};
  const RayCube cube = ray_cube(set.o_s, ds);
  bool hid = false;
  for (int j = 0; j < set.n; ++j) {
    float u_in, u_out, n[3];
    int which;
    ray_solid<false>(set.c[j], set.o_s, ds, cube, u_in, u_out, which, n);
    hid = hid || (u_in < u_out && u_out > 0.f && u_in < 1.f);
  }
  return hid;
}

__global__ void __launch_bounds__(kDrawThreads) k_collider_cast(int H, int W, DrawSet set, DrawStyles sty, RayBasis rb,
                                                                float* __restrict__ t_out, float* __restrict__ shade,
                                                                int32_t* __restrict__ hit) {
  const int px = blockIdx.x * kDrawThreads + threadIdx.x, py = blockIdx.y;
  if (px >= W) return;
  float best_t, rgb[3];
  int best;
  cast_pixel(px, py, H, W, set, sty, rb, best_t, best, rgb);
  const size_t p = (size_t)py * W + px, hw = (size_t)H * W;
  t_out[p] = best_t;
  hit[p] = best;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) shade[ch * hw + p] = rgb[ch];
}

__global__ void __launch_bounds__(kDrawThreads) k_collider_hide(int K, DrawSet set, float cx, float cy, float cz,
                                                                const float* __restrict__ means, const float* __restrict__ opacity,
                                                                float* __restrict__ opacity_front, uint8_t* __restrict__ hidden) {
  const int i = blockIdx.x * kDrawThreads + threadIdx.x;
  if (i >= K) return;
  const bool hid = hide_one(set, cx, cy, cz, means[3 * (size_t)i], means[3 * (size_t)i + 1], means[3 * (size_t)i + 2]);
  opacity_front[i] = hid ? 0.f : opacity[i];
  if (hidden) hidden[i] = hid ? 1 : 0;
}

__global__ void __launch_bounds__(kDrawThreads) k_collider_compose(int H, int W, int y0, int y1, const float* __restrict__ img_all,
                                                                   const float* __restrict__ rgb_front,
                                                                   const float* __restrict__ a_front, const float* __restrict__ shade,
                                                                   const int32_t* __restrict__ hit, float* __restrict__ out) {
  const int px = blockIdx.x * kDrawThreads + threadIdx.x, py = y0 + blockIdx.y;
  if (px >= W || py >= y1) return;
  const size_t p = (size_t)py * W + px, hw = (size_t)H * W;
  const bool h = hit[p] >= 0;
  const float keep = 1.f - a_front[p];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    out[ch * hw + p] = h ? rgb_front[ch * hw + p] + keep * shade[ch * hw + p] : img_all[ch * hw + p];
}

// ---------------------------------------------------------------- mesh (field) colliders: the sphere trace of nm_field_ray.h
// k_field_cast and k_field_hide work IN-OUT on what k_collider_cast / k_collider_hide have written: a field hit replaces a pixel
// only where its t is strictly smaller, a hidden Gaussian stays hidden.  The fields, their colours and the view travel by value;
// the loop over the fields is wave-uniform; no LDS, no atomics; a pixel that no field changes is not written.
struct FieldDrawSet {
  int n, hit_base;
  nm_field_collider c[NM_MAX_FIELD_COLLIDERS];
  float color[NM_MAX_FIELD_COLLIDERS][3];
  float a[3];         // render = a * sim + b, per axis
  float o_s[3];       // the camera in simulation coordinates: (campos - b) / a
};

// A wave is an 8x8 pixel tile, a workgroup four of them side by side: neighbouring rays take similar step counts and read
// neighbouring lattice cells (64 pixels of one row per wave, as in k_collider_cast, measured 412 us against 222 us: DESIGN.md)
__global__ void __launch_bounds__(kDrawThreads) k_field_cast(int H, int W, FieldDrawSet set, RayBasis rb, float* __restrict__ t_io,
                                                             float* __restrict__ shade, int32_t* __restrict__ hit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = (blockIdx.x * 4 + wave) * 8 + (lane & 7), py = blockIdx.y * 8 + (lane >> 3);
  if (px >= W || py >= H) return;
  const float nx = (float)(2 * px + 1) / (float)W - 1.f, ny = (float)(2 * py + 1) / (float)H - 1.f;
  float dr[3], ds[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) dr[a] = nx * rb.gx[a] + ny * rb.gy[a] + rb.g0[a];
  const float len = sqrtf(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dr[a] = dr[a] / len;
    ds[a] = dr[a] / set.a[a];
  }
  const float L = sqrtf(ds[0] * ds[0] + ds[1] * ds[1] + ds[2] * ds[2]);
  const RayCube cube = ray_cube(set.o_s, ds);
  const size_t p = (size_t)py * W + px, hw = (size_t)H * W;
  float best_t = t_io[p], rgb[3];      // what is in the buffer ends every march early
  int best = -1;
  for (int j = 0; j < set.n; ++j) {
    float t, n[3];
    int which;
    if (!field_trace<true>(set.c[j], set.o_s, ds, L, cube, best_t, t, which, n)) continue;
    if (!(t < best_t)) continue;      // (the polish may have moved t behind what is there)
    best_t = t;
    best = set.hit_base + j;
    const float nr0 = n[0] / set.a[0], nr1 = n[1] / set.a[1], nr2 = n[2] / set.a[2];
    const float nl = sqrtf(nr0 * nr0 + nr1 * nr1 + nr2 * nr2);
    float ndl = -(nr0 * dr[0] + nr1 * dr[1] + nr2 * dr[2]) / nl;
    ndl = which < 0 ? 1.f : ndl;      // the camera inside the solid: the normal faces the camera
    const float lam = 0.35f + 0.65f * fmaxf(0.f, ndl);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = set.color[j][ch] * lam;
  }
  if (best < 0) return;
  t_io[p] = best_t;
  hit[p] = best;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) shade[ch * hw + p] = rgb[ch];
}

__global__ void __launch_bounds__(kDrawThreads) k_field_hide(int K, FieldDrawSet set, float cx, float cy, float cz,
                                                             const float* __restrict__ means, float* __restrict__ opacity_front,
                                                             uint8_t* __restrict__ hidden) {
  const int i = blockIdx.x * kDrawThreads + threadIdx.x;
  if (i >= K) return;
  const float ds[3] = {(means[3 * (size_t)i] - cx) / set.a[0], (means[3 * (size_t)i + 1] - cy) / set.a[1],
                       (means[3 * (size_t)i + 2] - cz) / set.a[2]};
  const float L = sqrtf(ds[0] * ds[0] + ds[1] * ds[1] + ds[2] * ds[2]);
  const RayCube cube = ray_cube(set.o_s, ds);
  // the mean itself, for "the mean lies inside the solid": a march that ends at u >= 1 has not looked at u = 1
  const float m_s[3] = {set.o_s[0] + ds[0], set.o_s[1] + ds[1], set.o_s[2] + ds[2]};
  const bool in_cube = m_s[0] >= 0.f && m_s[0] <= 1.f && m_s[1] >= 0.f && m_s[1] <= 1.f && m_s[2] >= 0.f && m_s[2] <= 1.f;
  bool hid = false;
  for (int j = 0; j < set.n; ++j) {
    float u, n[3];
    int which;
    hid = hid || field_trace<false>(set.c[j], set.o_s, ds, L, cube, 1.f, u, which, n) || (in_cube && field_normal(set.c[j], m_s, n));
  }
  if (!hid) return;
  opacity_front[i] = 0.f;
  if (hidden) hidden[i] = 1;
}

bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// deterministic 2-D frame of a plane from its unit normal n (fp64): e = the coordinate axis along which |n| is smallest (the
// lowest index of equal ones), u = normalize(n x e), v = n x u
void plane_frame(const float* nf, float* u, float* v) {
  const double n[3] = {nf[0], nf[1], nf[2]};
  int e = 0;
  if (fabs(n[1]) < fabs(n[e])) e = 1;
  if (fabs(n[2]) < fabs(n[e])) e = 2;
  const double ev[3] = {e == 0 ? 1.0 : 0.0, e == 1 ? 1.0 : 0.0, e == 2 ? 1.0 : 0.0};
  double uu[3] = {n[1] * ev[2] - n[2] * ev[1], n[2] * ev[0] - n[0] * ev[2], n[0] * ev[1] - n[1] * ev[0]};
  const double l = sqrt(uu[0] * uu[0] + uu[1] * uu[1] + uu[2] * uu[2]);
  for (int a = 0; a < 3; ++a) uu[a] /= l;
  const double vv[3] = {n[1] * uu[2] - n[2] * uu[1], n[2] * uu[0] - n[0] * uu[2], n[0] * uu[1] - n[1] * uu[0]};
  for (int a = 0; a < 3; ++a) { u[a] = (float)uu[a]; v[a] = (float)vv[a]; }
}

// the checks of nm_mpm_set_colliders that matter for drawing, the map and the camera -> DrawSet
int make_set(const float* campos, const float* map_a, const float* map_b, int32_t n, const nm_collider* col, DrawSet* set) {
  NM_REQUIRE(campos && map_a && map_b, "campos, map_a and map_b must not be NULL");
  NM_REQUIREF(n >= 0 && n <= NM_MAX_COLLIDERS, "colliders: n = %d outside 0..%d", (int)n, NM_MAX_COLLIDERS);
  NM_REQUIRE(n == 0 || col, "colliders: NULL with n > 0");
  NM_REQUIRE(finite3(campos), "campos: not finite");
  NM_REQUIRE(finite3(map_b), "map_b: not finite");
  NM_REQUIREF(finite3(map_a) && map_a[0] > 0.f && map_a[1] > 0.f && map_a[2] > 0.f, "map_a: a <= 0 or not finite (%g, %g, %g)",
              (double)map_a[0], (double)map_a[1], (double)map_a[2]);
  memset(set, 0, sizeof(*set));
  set->n = n;
  for (int i = 0; i < n; ++i) {
    const nm_collider& c = col[i];
    NM_REQUIREF(c.shape >= NM_COLLIDER_PLANE && c.shape <= NM_COLLIDER_BOX, "collider %d: shape: unknown shape %d", i, (int)c.shape);
    NM_REQUIREF(finite3(c.center), "collider %d: center: not finite", i);
    if (c.shape == NM_COLLIDER_PLANE) {
      const double l2 = (double)c.normal[0] * c.normal[0] + (double)c.normal[1] * c.normal[1] + (double)c.normal[2] * c.normal[2];
      NM_REQUIREF(finite3(c.normal) && fabs(sqrt(l2) - 1.0) <= 1e-4, "collider %d: normal: not a unit vector", i);
    } else if (c.shape == NM_COLLIDER_SPHERE) {
      NM_REQUIREF(isfinite(c.radius) && c.radius > 0.f, "collider %d: radius: must be positive", i);
    } else {
      NM_REQUIREF(finite3(c.half) && c.half[0] > 0.f && c.half[1] > 0.f && c.half[2] > 0.f, "collider %d: half: extents must be positive", i);
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double dd = 0.0;
          for (int r = 0; r < 3; ++r) dd += (double)c.rot[3 * r + a] * c.rot[3 * r + b];
          NM_REQUIREF(fabs(dd - (a == b ? 1.0 : 0.0)) <= 1e-4, "collider %d: rot: not orthonormal", i);
        }
    }
    set->c[i] = c;
  }
  for (int a = 0; a < 3; ++a) {
    set->a[a] = map_a[a];
    set->o_s[a] = (float)(((double)campos[a] - (double)map_b[a]) / (double)map_a[a]);
  }
  return NM_OK;
}

// the styles (with the planes' frames) and the ray basis of one view
int make_view(const nm_raster_cfg* cfg, const double* inv_proj, int32_t n, const nm_collider* colliders, const nm_collider_style* styles,
              DrawStyles* sty, RayBasis* rb) {
  NM_REQUIRE(n == 0 || styles, "styles: NULL with n > 0");
  memset(sty, 0, sizeof(*sty));
  for (int i = 0; i < n; ++i) {
    const nm_collider_style& s = styles[i];
    NM_REQUIREF(finite3(s.color), "style %d: color: not finite", i);
    NM_REQUIREF(isfinite(s.checker) && s.checker >= 0.f, "style %d: checker: must be finite and not negative", i);
    for (int a = 0; a < 3; ++a) sty->s[i].color[a] = s.color[a];
    sty->s[i].checker = s.checker;
    if (colliders[i].shape == NM_COLLIDER_PLANE) plane_frame(colliders[i].normal, sty->s[i].u, sty->s[i].v);
  }
  // hom = (x, y, z, 1) inv_proj (row vector, as the rasterizer's projmatrix) is a point that projects to ndc (x, y, z); with the
  // far-plane row R = row 2 + row 3 folded here in fp64, hom.xyz - hom.w campos is the ray's direction times a positive number
  for (int a = 0; a < 3; ++a) {
    const double c = (double)cfg->campos[a];
    NM_REQUIRE(isfinite(inv_proj[a]) && isfinite(inv_proj[4 + a]) && isfinite(inv_proj[8 + a]) && isfinite(inv_proj[12 + a]) &&
                   isfinite(inv_proj[3]) && isfinite(inv_proj[7]) && isfinite(inv_proj[11]) && isfinite(inv_proj[15]),
               "inv_proj: not finite");
    rb->gx[a] = (float)(inv_proj[a] - inv_proj[3] * c);
    rb->gy[a] = (float)(inv_proj[4 + a] - inv_proj[7] * c);
    rb->g0[a] = (float)((inv_proj[8 + a] + inv_proj[12 + a]) - (inv_proj[11] + inv_proj[15]) * c);
  }
  return NM_OK;
}

// rows [y0, y1) of the nm_raster_cfg's stripe (tile rows of 16 pixels; tile_y1 <= tile_y0: the whole image)
void stripe_rows(const nm_raster_cfg* cfg, int* y0, int* y1) {
  const int H = cfg->image_height;
  if (cfg->tile_y1 <= cfg->tile_y0) { *y0 = 0; *y1 = H; return; }
  *y0 = cfg->tile_y0 * 16 < H ? cfg->tile_y0 * 16 : H;
  *y1 = cfg->tile_y1 * 16 < H ? cfg->tile_y1 * 16 : H;
}

// the checks of nm_mpm_set_field_colliders, the map and the camera -> FieldDrawSet (colours and hit_base: the caller)
int make_field_set(const float* campos, const float* map_a, const float* map_b, int32_t n, const nm_field_collider* fields,
                   FieldDrawSet* set) {
  NM_REQUIRE(campos && map_a && map_b, "campos, map_a and map_b must not be NULL");
  NM_REQUIREF(n >= 0 && n <= NM_MAX_FIELD_COLLIDERS, "field colliders: n = %d outside 0..%d", (int)n, NM_MAX_FIELD_COLLIDERS);
  NM_REQUIRE(n == 0 || fields, "field colliders: NULL with n > 0");
  NM_REQUIRE(finite3(campos), "campos: not finite");
  NM_REQUIRE(finite3(map_b), "map_b: not finite");
  NM_REQUIREF(finite3(map_a) && map_a[0] > 0.f && map_a[1] > 0.f && map_a[2] > 0.f, "map_a: a <= 0 or not finite (%g, %g, %g)",
              (double)map_a[0], (double)map_a[1], (double)map_a[2]);
  memset(set, 0, sizeof(*set));
  set->n = n;
  for (int q = 0; q < n; ++q) {
    const nm_field_collider& c = fields[q];
    NM_REQUIREF(c.surface == NM_SURFACE_STICKY || c.surface == NM_SURFACE_SLIP || c.surface == NM_SURFACE_FRICTION,
                "field collider %d: surface: unknown surface %d", q, (int)c.surface);
    NM_REQUIREF(c.friction >= 0.f && isfinite(c.friction), "field collider %d: friction: must not be negative", q);
    NM_REQUIREF(finite3(c.velocity), "field collider %d: velocity: three finite numbers expected", q);
    NM_REQUIREF(finite3(c.origin), "field collider %d: origin: three finite numbers expected", q);
    NM_REQUIREF(c.spacing > 0.f && isfinite(c.spacing), "field collider %d: spacing: must be positive", q);
    NM_REQUIREF(c.dims[0] >= 2 && c.dims[1] >= 2 && c.dims[2] >= 2, "field collider %d: dims: every lattice size must be >= 2", q);
    const int64_t lim = (int64_t)1 << 27;
    NM_REQUIREF(c.dims[0] <= lim && c.dims[1] <= lim && (int64_t)c.dims[0] * c.dims[1] <= lim &&
                    (int64_t)c.dims[0] * c.dims[1] * c.dims[2] <= lim,
                "field collider %d: dims: more than 2^27 nodes", q);
    NM_REQUIREF(c.phi != nullptr, "field collider %d: phi: null pointer", q);
    set->c[q] = c;
  }
  for (int a = 0; a < 3; ++a) {
    set->a[a] = map_a[a];
    set->o_s[a] = (float)(((double)campos[a] - (double)map_b[a]) / (double)map_a[a]);
  }
  return NM_OK;
}

}  // namespace

extern "C" int nm_collider_cast(const nm_raster_cfg* cfg, const double* inv_proj, const float* map_a, const float* map_b, int32_t n,
                                const nm_collider* colliders, const nm_collider_style* styles, float* t, float* shade, int32_t* hit,
                                void* stream) {
  NM_REQUIRE(cfg && inv_proj, "cfg and inv_proj must not be NULL");
  NM_REQUIRE(cfg->image_height > 0 && cfg->image_width > 0, "cfg: image size must be positive");
  NM_REQUIRE(t && shade && hit, "t, shade and hit must not be NULL");
  DrawSet set;
  if (int rc = make_set(cfg->campos, map_a, map_b, n, colliders, &set)) return rc;
  DrawStyles sty;
  RayBasis rb;
  if (int rc = make_view(cfg, inv_proj, n, colliders, styles, &sty, &rb)) return rc;
  const int H = cfg->image_height, W = cfg->image_width;
  NM_LAUNCH(k_collider_cast, dim3(nm_div_up(W, kDrawThreads), H), dim3(kDrawThreads), 0, (hipStream_t)stream, H, W, set, sty, rb, t,
            shade, hit);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_collider_hide(const float* campos, const float* map_a, const float* map_b, int32_t n, const nm_collider* colliders,
                                int32_t k, const float* means3D, const float* opacity, float* opacity_front, uint8_t* hidden,
                                void* stream) {
  DrawSet set;
  if (int rc = make_set(campos, map_a, map_b, n, colliders, &set)) return rc;
  NM_REQUIRE(k >= 0, "k < 0");
  if (k == 0) return NM_OK;
  NM_REQUIRE(means3D && opacity && opacity_front, "means3D, opacity and opacity_front must not be NULL");
  NM_LAUNCH(k_collider_hide, dim3(nm_div_up(k, kDrawThreads)), dim3(kDrawThreads), 0, (hipStream_t)stream, (int)k, set, campos[0],
            campos[1], campos[2], means3D, opacity, opacity_front, hidden);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_collider_compose(const nm_raster_cfg* cfg, const float* img_all, const float* rgb_front, const float* a_front,
                                   const float* shade, const int32_t* hit, float* out, void* stream) {
  NM_REQUIRE(cfg, "cfg must not be NULL");
  NM_REQUIRE(cfg->image_height > 0 && cfg->image_width > 0, "cfg: image size must be positive");
  NM_REQUIRE(img_all && rgb_front && a_front && shade && hit && out, "img_all, rgb_front, a_front, shade, hit and out must not be NULL");
  int y0, y1;
  stripe_rows(cfg, &y0, &y1);
  if (y1 <= y0) return NM_OK;
  NM_LAUNCH(k_collider_compose, dim3(nm_div_up(cfg->image_width, kDrawThreads), y1 - y0), dim3(kDrawThreads), 0, (hipStream_t)stream,
            cfg->image_height, cfg->image_width, y0, y1, img_all, rgb_front, a_front, shade, hit, out);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_collider_cast_field(const nm_raster_cfg* cfg, const double* inv_proj, const float* map_a, const float* map_b, int32_t n,
                                      const nm_field_collider* fields, const nm_collider_style* styles, int32_t hit_base, float* t,
                                      float* shade, int32_t* hit, void* stream) {
  NM_REQUIRE(cfg && inv_proj, "cfg and inv_proj must not be NULL");
  NM_REQUIRE(cfg->image_height > 0 && cfg->image_width > 0, "cfg: image size must be positive");
  NM_REQUIRE(t && shade && hit, "t, shade and hit must not be NULL");
  NM_REQUIREF(hit_base >= 0, "hit_base: %d is negative", (int)hit_base);
  FieldDrawSet set;
  if (int rc = make_field_set(cfg->campos, map_a, map_b, n, fields, &set)) return rc;
  DrawStyles sty;      // (the colours and the ray basis, through the checks of nm_collider_cast; no field is a plane)
  RayBasis rb;
  nm_collider none[NM_MAX_FIELD_COLLIDERS];
  for (int i = 0; i < NM_MAX_FIELD_COLLIDERS; ++i) none[i].shape = NM_COLLIDER_SPHERE;
  if (int rc = make_view(cfg, inv_proj, n, none, styles, &sty, &rb)) return rc;
  if (n == 0) return NM_OK;
  set.hit_base = hit_base;
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) set.color[i][a] = sty.s[i].color[a];
  const int H = cfg->image_height, W = cfg->image_width;
  NM_LAUNCH(k_field_cast, dim3(nm_div_up(W, 32), nm_div_up(H, 8)), dim3(kDrawThreads), 0, (hipStream_t)stream, H, W, set, rb, t, shade, hit);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

extern "C" int nm_collider_hide_field(const float* campos, const float* map_a, const float* map_b, int32_t n,
                                      const nm_field_collider* fields, int32_t k, const float* means3D, float* opacity_front,
                                      uint8_t* hidden, void* stream) {
  FieldDrawSet set;
  if (int rc = make_field_set(campos, map_a, map_b, n, fields, &set)) return rc;
  NM_REQUIRE(k >= 0, "k < 0");
  if (k == 0 || n == 0) return NM_OK;
  NM_REQUIRE(means3D && opacity_front, "means3D and opacity_front must not be NULL");
  NM_LAUNCH(k_field_hide, dim3(nm_div_up(k, kDrawThreads)), dim3(kDrawThreads), 0, (hipStream_t)stream, (int)k, set, campos[0], campos[1],
            campos[2], means3D, opacity_front, hidden);
  NM_LAUNCH_CHECK();
  return NM_OK;
}
