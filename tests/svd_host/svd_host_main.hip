// Stand-alone driver for the HOST half of nm_svd3 / nm_svd3_adj (both are __host__ __device__): no HIP call, no GPU.
//   svd_host_main F.bin OUT.bin [G.bin]
// F.bin   : int32 n, then n x 9 floats (row-major 3x3)
// G.bin   : n x 9 gU | n x 3 gsigma | n x 9 gVh (optional: also run the adjoint on the factors just computed)
// OUT.bin : n x 9 U | n x 3 sigma | n x 9 V | (with G.bin) n x 9 gF
// tests/test_svd_host_cpu.py builds and runs it; it is also the target for a host sanitizer build.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../neuma_amd/csrc/nm_common.h"

static bool read_exact(FILE* f, void* dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    fprintf(stderr, "usage: %s F.bin OUT.bin [G.bin]\n", argv[0]);
    return 2;
  }
  FILE* fin = fopen(argv[1], "rb");
  if (!fin) { perror(argv[1]); return 1; }
  int32_t n = 0;
  if (!read_exact(fin, &n, sizeof n) || n < 0 || n > (1 << 24)) { fprintf(stderr, "bad header in %s\n", argv[1]); return 1; }
  std::vector<float> F((size_t)n * 9);
  if (!read_exact(fin, F.data(), F.size() * sizeof(float))) { fprintf(stderr, "short read of %s\n", argv[1]); return 1; }
  fclose(fin);
  std::vector<float> G;
  if (argc == 4) {
    G.resize((size_t)n * 21);
    FILE* fg = fopen(argv[3], "rb");
    if (!fg) { perror(argv[3]); return 1; }
    if (!read_exact(fg, G.data(), G.size() * sizeof(float))) { fprintf(stderr, "short read of %s\n", argv[3]); return 1; }
    fclose(fg);
  }
  std::vector<float> U((size_t)n * 9), S((size_t)n * 3), V((size_t)n * 9), gF(G.empty() ? 0 : (size_t)n * 9);
  for (int32_t p = 0; p < n; ++p) {
    M3 A = m3_load(F.data() + 9 * (size_t)p), Um, Vm;
    float s[3];
    nm_svd3(A, Um, s, Vm);
    m3_store(U.data() + 9 * (size_t)p, Um);
    m3_store(V.data() + 9 * (size_t)p, Vm);
    for (int k = 0; k < 3; ++k) S[3 * (size_t)p + k] = s[k];
    if (!G.empty()) {
      const float* gU = G.data() + 9 * (size_t)p;
      const float* gs = G.data() + (size_t)n * 9 + 3 * (size_t)p;
      const float* gVh = G.data() + (size_t)n * 12 + 9 * (size_t)p;
      float g[3] = {gs[0], gs[1], gs[2]};
      m3_store(gF.data() + 9 * (size_t)p, nm_svd3_adj(Um, s, m3_transpose(Vm), m3_load(gU), g, m3_load(gVh)));
    }
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  bool ok = fwrite(U.data(), sizeof(float), U.size(), fo) == U.size() && fwrite(S.data(), sizeof(float), S.size(), fo) == S.size() &&
            fwrite(V.data(), sizeof(float), V.size(), fo) == V.size() &&
            fwrite(gF.data(), sizeof(float), gF.size(), fo) == gF.size();
  ok = (fclose(fo) == 0) && ok;
  if (!ok) { fprintf(stderr, "short write of %s\n", argv[2]); return 1; }
  return 0;
}
