// TEST INFRASTRUCTURE: a stand-alone host program around pl::dyn_jac_point (csrc/dyn_jac.h, the
// columns k_dyn_jac runs), so that the CPU suite can run the Jacobian columns' host code under
// AddressSanitizer / UBSan directly, with nothing loaded into python (tests/test_dyn_jac_host.py).
// Not linked into the product.
//
// Input file (argv[1]), native byte order: int32 sizeof(PlModel), sizeof(PlOcpConst), ncases; the
// PlModel and PlOcpConst bytes (pl_debug_consts of a host OCP handle: its contact frames are the
// plugin handle's); then per case int32 fn, flags, frame (0 none, 1 the first foot, 2 the arm
// frame), wrt, and the inputs the function takes as doubles (lengths from pl::dyn_in_len).
// Prints every case's Jacobian, row-major [rows][W], one value per line (%.17g).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dyn_jac.h"

static void rd(FILE* f, void* dst, size_t bytes) {
  if (fread(dst, 1, bytes, f) != bytes) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[3];
  rd(f, hd, sizeof(hd));
  if (hd[0] != (int)sizeof(PlModel) || hd[1] != (int)sizeof(PlOcpConst)) {
    fprintf(stderr, "struct sizes differ from the library's\n");
    return 2;
  }
  // on the heap, exactly sized: the sanitizer sees every read past an end
  std::vector<PlModel> M(1);
  std::vector<PlOcpConst> O(1);
  rd(f, M.data(), sizeof(PlModel));
  rd(f, O.data(), sizeof(PlOcpConst));
  for (int cs = 0; cs < hd[2]; ++cs) {
    int c4[4];
    rd(f, c4, sizeof(c4));
    const int fn = c4[0], flags = c4[1], frame = c4[2];
    const unsigned wrt = (unsigned)c4[3];
    if (pl::dyn_jac_family(fn) == pl::PL_JF_NONE) {
      fprintf(stderr, "function %d has no Jacobian\n", fn);
      return 2;
    }
    int len[4], tan[4], W = 0;
    pl::dyn_jac_tan_len(M[0], fn, O[0].nf, len, tan);
    std::vector<std::vector<double>> in(4);
    for (int k = 0; k < 4; ++k) {
      in[k].resize(len[k]);
      if (len[k]) rd(f, in[k].data(), len[k] * sizeof(double));
      if ((wrt >> k) & 1u) W += tan[k];
    }
    std::vector<PlFrameRef> F(1);
    F[0] = frame == 2 ? O[0].arm : O[0].feet[0];
    const int rows = pl::dyn_jac_rows(M[0], fn);
    std::vector<double> jac((size_t)rows * W, 0.0);
    pl::dyn_jac_point(M[0], O[0], F[0], fn, flags, wrt, len[0] ? in[0].data() : nullptr, len[1] ? in[1].data() : nullptr,
                      len[2] ? in[2].data() : nullptr, len[3] ? in[3].data() : nullptr, jac.data());
    for (double v : jac) printf("%.17g\n", v);
  }
  fclose(f);
  return 0;
}
