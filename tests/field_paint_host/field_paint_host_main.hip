// Stand-alone driver for the HOST half of the field paint (nm_particle_field_one and nm_field_color are __host__ __device__): no HIP
// call, no GPU.
//   field_paint_host_main field IN.bin OUT.bin
//     IN.bin  : int32 n, int32 quantity (NM_FIELD_*), then x (n x 3) | v (n x 3) | F (n x 9) | stress (n x 9) | x0 (n x 3), fp32
//     OUT.bin : n floats q
//   field_paint_host_main color IN.bin OUT.bin
//     IN.bin  : int32 n, int32 n_knots, float lo, float hi, 24 floats knots (the first 3 n_knots are read), 3 floats no-data rgb,
//               then n floats g
//     OUT.bin : n x 3 SH DC coefficients
// tests/test_field_paint_cpu.py builds and runs it; it is also the target for a host sanitizer build.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../neuma_amd/csrc/nm_particle_field.h"

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static bool write_floats(const char* path, const std::vector<float>& a) {
  FILE* fo = fopen(path, "wb");
  if (!fo) { perror(path); return false; }
  bool ok = fwrite(a.data(), sizeof(float), a.size(), fo) == a.size();
  ok = (fclose(fo) == 0) && ok;
  if (!ok) fprintf(stderr, "short write of %s\n", path);
  return ok;
}

template <int Q>
static void run_field(int32_t n, const float* x, const float* v, const float* F, const float* S, const float* x0, float* q) {
  for (int32_t p = 0; p < n; ++p)
    q[p] = nm_particle_field_one<Q>(x + 3 * (size_t)p, v + 3 * (size_t)p, m3_load(F + 9 * (size_t)p), m3_load(S + 9 * (size_t)p),
                                    x0 + 3 * (size_t)p);
}

static int main_field(FILE* fin, const char* in, const char* out) {
  int32_t n = 0, quantity = -1;
  if (!read_exact(fin, &n, sizeof n) || !read_exact(fin, &quantity, sizeof quantity) || n < 0 || n > (1 << 24) || quantity < 0 ||
      quantity >= NM_FIELD_COUNT) {
    fprintf(stderr, "bad header in %s\n", in);
    return 1;
  }
  const size_t N = (size_t)n;
  std::vector<float> x(3 * N), v(3 * N), F(9 * N), S(9 * N), x0(3 * N), q(N);
  if (!read_exact(fin, x.data(), 12 * N) || !read_exact(fin, v.data(), 12 * N) || !read_exact(fin, F.data(), 36 * N) ||
      !read_exact(fin, S.data(), 36 * N) || !read_exact(fin, x0.data(), 12 * N)) {
    fprintf(stderr, "short read of %s\n", in);
    return 1;
  }
  switch (quantity) {
    case NM_FIELD_SPEED: run_field<NM_FIELD_SPEED>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
    case NM_FIELD_DISPLACEMENT: run_field<NM_FIELD_DISPLACEMENT>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
    case NM_FIELD_VOLUME: run_field<NM_FIELD_VOLUME>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
    case NM_FIELD_STRAIN: run_field<NM_FIELD_STRAIN>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
    case NM_FIELD_PRESSURE: run_field<NM_FIELD_PRESSURE>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
    default: run_field<NM_FIELD_VON_MISES>(n, x.data(), v.data(), F.data(), S.data(), x0.data(), q.data()); break;
  }
  return write_floats(out, q) ? 0 : 1;
}

static int main_color(FILE* fin, const char* in, const char* out) {
  int32_t n = 0, nk = 0;
  float lo = 0.f, hi = 1.f, knots[3 * NM_PAINT_MAX_KNOTS], nodata[3];
  if (!read_exact(fin, &n, sizeof n) || !read_exact(fin, &nk, sizeof nk) || !read_exact(fin, &lo, sizeof lo) ||
      !read_exact(fin, &hi, sizeof hi) || !read_exact(fin, knots, sizeof knots) || !read_exact(fin, nodata, sizeof nodata) || n < 0 ||
      n > (1 << 24) || nk < 2 || nk > NM_PAINT_MAX_KNOTS) {
    fprintf(stderr, "bad header in %s\n", in);
    return 1;
  }
  std::vector<float> g((size_t)n), dc(3 * (size_t)n);
  if (!read_exact(fin, g.data(), 4 * (size_t)n)) {
    fprintf(stderr, "short read of %s\n", in);
    return 1;
  }
  NmPaintMap map;
  memset(&map, 0, sizeof map);
  map.n = nk;
  for (int a = 0; a < 3 * nk; ++a) map.c[a / 3][a % 3] = knots[a];
  for (int a = 0; a < 3; ++a) map.nodata[a] = nodata[a];
  for (int32_t p = 0; p < n; ++p) nm_field_color(g[p], lo, hi, map, dc.data() + 3 * (size_t)p);
  return write_floats(out, dc) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "field") != 0 && strcmp(argv[1], "color") != 0)) {
    fprintf(stderr, "usage: %s field|color IN.bin OUT.bin\n", argv[0]);
    return 2;
  }
  FILE* fin = fopen(argv[2], "rb");
  if (!fin) { perror(argv[2]); return 1; }
  const int rc = argv[1][0] == 'f' ? main_field(fin, argv[2], argv[3]) : main_color(fin, argv[2], argv[3]);
  fclose(fin);
  return rc;
}
