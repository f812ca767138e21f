// TEST INFRASTRUCTURE: a stand-alone host program around pl::plant_step with contact (csrc/plant.h),
// so that the CPU suite can run the plant's host code under AddressSanitizer / UBSan directly,
// with nothing loaded into python (tests/test_contact_sanitize.py).  Not linked into the product.
//
// Input file (argv[1]), native byte order: int32 sizeof(PlModel), sizeof(PlOcpConst), N, np, n, nx,
// substeps, calls; then the PlModel and PlOcpConst bytes (pl_debug_consts), int32 x_off[N + 1]
// (pl_debug_nodes), and doubles p[np], x[n], x_state[nx], wrench[6], contact[8], ground_z[n_feet].
// Runs `calls` plant steps (the anchors carried along) and prints x_state, anchors and the last
// ground forces, one value per line (%.17g).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plant.h"

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
  int hd[8];
  rd(f, hd, sizeof(hd));
  if (hd[0] != (int)sizeof(PlModel) || hd[1] != (int)sizeof(PlOcpConst)) {
    fprintf(stderr, "struct sizes differ from the library's\n");
    return 2;
  }
  const int N = hd[2], np = hd[3], n = hd[4], nx = hd[5], substeps = hd[6], calls = hd[7];
  // on the heap, exactly sized: the sanitizer sees every read past an end
  std::vector<PlModel> M(1);
  std::vector<PlOcpConst> O(1);
  rd(f, M.data(), sizeof(PlModel));
  rd(f, O.data(), sizeof(PlOcpConst));
  std::vector<int> xoff(N + 1);
  rd(f, xoff.data(), xoff.size() * sizeof(int));
  std::vector<PlNode> nodes(N + 1);
  for (int i = 0; i <= N; ++i) {
    nodes[i] = PlNode{};
    nodes[i].x_off = xoff[i];
  }
  const int nfeet = O[0].nfeet;
  std::vector<double> p(np), x(n), xs(nx), w(6), c8(8), gz(nfeet), anchors(3 * nfeet, 0.0), fg(3 * nfeet, 0.0);
  rd(f, p.data(), np * 8);
  rd(f, x.data(), n * 8);
  rd(f, xs.data(), nx * 8);
  rd(f, w.data(), 6 * 8);
  rd(f, c8.data(), 8 * 8);
  rd(f, gz.data(), nfeet * 8);
  fclose(f);
  const PlContact c{c8[0], c8[1], c8[2], c8[3], c8[4], c8[5], c8[6], c8[7]};
  for (int k = 0; k < calls; ++k)
    pl::plant_step<true>(M[0], O[0], O[0].dyn, nodes.data(), N, p.data(), x.data(), w.data(), substeps, xs.data(), &c,
                         gz.data(), anchors.data(), fg.data());
  for (double v : xs) printf("%.17g\n", v);
  for (double v : anchors) printf("%.17g\n", v);
  for (double v : fg) printf("%.17g\n", v);
  return 0;
}
