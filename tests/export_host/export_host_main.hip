// Stand-alone driver for the HOST half of nm_gaussian_deform_one (__host__ __device__, as nm_svd3 is): no HIP call, no GPU.
//   export_host_main IN.bin OUT.bin
// IN.bin  : int32 n, int32 has_F, float scale_modifier, then n x 3 log-scales | n x 4 raw quaternions | (has_F) n x 9 F (row-major)
// OUT.bin : n x 3 log-scales' | n x 4 quaternions'
// tests/test_gaussian_export_cpu.py builds and runs it; it is also the target for a host sanitizer build.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../neuma_amd/csrc/nm_gaussian_deform.h"

static bool read_exact(FILE* f, void* dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN.bin OUT.bin\n", argv[0]);
    return 2;
  }
  FILE* fin = fopen(argv[1], "rb");
  if (!fin) { perror(argv[1]); return 1; }
  int32_t n = 0, has_F = 0;
  float mod = 1.f;
  if (!read_exact(fin, &n, sizeof n) || !read_exact(fin, &has_F, sizeof has_F) || !read_exact(fin, &mod, sizeof mod) || n < 0 ||
      n > (1 << 24) || (has_F != 0 && has_F != 1)) {
    fprintf(stderr, "bad header in %s\n", argv[1]);
    return 1;
  }
  std::vector<float> ls((size_t)n * 3), rot((size_t)n * 4), F(has_F ? (size_t)n * 9 : 0);
  if (!read_exact(fin, ls.data(), ls.size() * sizeof(float)) || !read_exact(fin, rot.data(), rot.size() * sizeof(float)) ||
      !read_exact(fin, F.data(), F.size() * sizeof(float))) {
    fprintf(stderr, "short read of %s\n", argv[1]);
    return 1;
  }
  fclose(fin);
  std::vector<float> lo((size_t)n * 3), qo((size_t)n * 4);
  for (int32_t p = 0; p < n; ++p)
    nm_gaussian_deform_one(ls.data() + 3 * (size_t)p, rot.data() + 4 * (size_t)p, has_F ? F.data() + 9 * (size_t)p : nullptr, mod,
                           lo.data() + 3 * (size_t)p, qo.data() + 4 * (size_t)p);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  bool ok = fwrite(lo.data(), sizeof(float), lo.size(), fo) == lo.size() && fwrite(qo.data(), sizeof(float), qo.size(), fo) == qo.size();
  ok = (fclose(fo) == 0) && ok;
  if (!ok) { fprintf(stderr, "short write of %s\n", argv[2]); return 1; }
  return 0;
}
