// Stand-alone driver for the HOST half of nm_cells_fit / nm_cell (both are __host__ __device__): no HIP call, no GPU.
//   cells_host_main IN.bin OUT.bin
// IN.bin  : doubles: D (2 or 3), n, P, then n records of lo[D] | hi[D] | cmax | P probe coordinates for each of the D axes
// OUT.bin : doubles: per record lo[D] | hi[D] (as the fit rewrote them) | extent[D] | o[D] | inv_h[D] | n[D] |
//           nm_cell of every probe against its axis (D x P)
// tests/test_cells_host_cpu.py builds and runs it; it is also the target for a host sanitizer build.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../neuma_amd/csrc/nm_cells.h"

template <int D>
static void run(const double* in, size_t n, size_t P, std::vector<double>& out) {
  const size_t rec = 2 * D + 1 + D * P;
  for (size_t r = 0; r < n; ++r) {
    const double* q = in + r * rec;
    double lo[D], hi[D], e[D];
    for (int k = 0; k < D; ++k) { lo[k] = q[k]; hi[k] = q[D + k]; }
    NmCells<D> c;
    nm_cells_fit(lo, hi, (int)q[2 * D], c, e);
    for (int k = 0; k < D; ++k) out.push_back(lo[k]);
    for (int k = 0; k < D; ++k) out.push_back(hi[k]);
    for (int k = 0; k < D; ++k) out.push_back(e[k]);
    for (int k = 0; k < D; ++k) out.push_back(c.o[k]);
    for (int k = 0; k < D; ++k) out.push_back(c.inv_h[k]);
    for (int k = 0; k < D; ++k) out.push_back((double)c.n[k]);
    for (int k = 0; k < D; ++k)
      for (size_t p = 0; p < P; ++p) out.push_back((double)nm_cell(q[2 * D + 1 + k * P + p], c.o[k], c.inv_h[k], c.n[k]));
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN.bin OUT.bin\n", argv[0]);
    return 2;
  }
  FILE* fin = fopen(argv[1], "rb");
  if (!fin) { perror(argv[1]); return 1; }
  double head[3];
  if (fread(head, sizeof(double), 3, fin) != 3 || !(head[0] == 2 || head[0] == 3) || !(head[1] >= 0 && head[1] <= 1 << 20) ||
      !(head[2] >= 0 && head[2] <= 1024)) {
    fprintf(stderr, "bad header in %s\n", argv[1]);
    return 1;
  }
  const int D = (int)head[0];
  const size_t n = (size_t)head[1], P = (size_t)head[2];
  std::vector<double> in(n * (2 * D + 1 + D * P)), out;
  if (fread(in.data(), sizeof(double), in.size(), fin) != in.size()) { fprintf(stderr, "short read of %s\n", argv[1]); return 1; }
  fclose(fin);
  for (size_t r = 0; r < n; ++r) {
    const double cmax = in[r * (2 * D + 1 + D * P) + 2 * D];
    if (!(cmax >= 1 && cmax <= 2147483647.0)) { fprintf(stderr, "record %zu: budget out of range\n", r); return 1; }
  }
  if (D == 2) run<2>(in.data(), n, P, out);
  else run<3>(in.data(), n, P, out);
  FILE* fout = fopen(argv[2], "wb");
  if (!fout) { perror(argv[2]); return 1; }
  const bool ok = fwrite(out.data(), sizeof(double), out.size(), fout) == out.size();
  return fclose(fout) == 0 && ok ? 0 : 1;
}
