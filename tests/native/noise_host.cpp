// TEST INFRASTRUCTURE: a stand-alone host program around pl::noise_prepare_host (csrc/noise.h), the
// body of pl_mpc_noise_host and the code k_mpc_prepare runs while pl_mpc_set_noise holds seeds, so
// that the CPU suite can run it under AddressSanitizer / UBSan directly, with nothing loaded into
// python (tests/test_noise_host.py).  Not linked into the product.
//
// Input file (argv[1]), native byte order: int32 sizeof(PlModel), sizeof(PlOcpConst), nx, ndx,
// steps; then the PlModel and PlOcpConst bytes (pl_debug_consts); uint64 seed; doubles
// state_sigma[ndx], wrench_sigma[6], det_wrench[6], x_state[nx]; int32 k[steps].
// Every array sits in a heap block of exactly its length: a read or a write past a component
// count is a sanitizer report.  Prints, first, the Philox block of the counter (k[0], 0, 0, 0)
// under the seed's key as four integers, then per step state_noise[ndx], base_wrench[6] and
// x_init[nx], one value per line (%.17g).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "noise.h"

static void rd(FILE* f, void* dst, size_t bytes) {
  if (bytes && fread(dst, 1, bytes, f) != bytes) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[5];
  rd(f, hd, sizeof(hd));
  if (hd[0] != (int)sizeof(PlModel) || hd[1] != (int)sizeof(PlOcpConst)) {
    fprintf(stderr, "struct sizes differ from the library's\n");
    return 2;
  }
  const int nx = hd[2], ndx = hd[3], steps = hd[4];
  std::vector<PlModel> M(1);
  std::vector<PlOcpConst> O(1);
  rd(f, M.data(), sizeof(PlModel));
  rd(f, O.data(), sizeof(PlOcpConst));
  if (O[0].ndx != ndx) {
    fprintf(stderr, "ndx differs from the descriptor's\n");
    return 2;
  }
  std::vector<unsigned long long> seed(1);
  rd(f, seed.data(), 8);
  std::vector<double> sig(ndx), wsig(6), det(6), xs(nx);
  rd(f, sig.data(), (size_t)ndx * 8);
  rd(f, wsig.data(), 6 * 8);
  rd(f, det.data(), 6 * 8);
  rd(f, xs.data(), (size_t)nx * 8);
  std::vector<int> ks(steps);
  rd(f, ks.data(), steps * sizeof(int));
  fclose(f);
  std::vector<uint32_t> w(4);
  pl::rng_block(seed[0], (uint32_t)(steps ? ks[0] : 0), 0u, 0u, 0u, w.data());
  for (uint32_t v : w) printf("%u\n", v);
  for (int s = 0; s < steps; ++s) {
    std::vector<double> z(ndx), bw(6), xi(nx);
    pl::noise_prepare_host(M[0], O[0], nx, ks[s], seed[0], sig.data(), wsig.data(), det.data(), xs.data(), z.data(),
                           bw.data(), xi.data());
    for (double v : z) printf("%.17g\n", v);
    for (double v : bw) printf("%.17g\n", v);
    for (double v : xi) printf("%.17g\n", v);
  }
  return 0;
}
