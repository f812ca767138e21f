// TEST INFRASTRUCTURE: a stand-alone host program around pl::record_host (csrc/record.h), the
// body of pl_mpc_record_host and the code k_mpc_record runs, so that the CPU suite can run it under
// AddressSanitizer / UBSan directly, with nothing loaded into python
// (tests/test_rollout_host.py).  Not linked into the product.
//
// Input file (argv[1]), native byte order: int32 nx, nu0, n_feet, qoff, capacity, every, steps,
// tolerance flags (bit 0: dz_tol given, bit 1: cz_min given); doubles z_ref, dz_tol, cz_min; then
// per step doubles k, x_init[nx], u0[nu0], stats[8] (status, admm_iters, ls_accepted, ls_alpha,
// viol_max, f, pri_res, dua_res), x_state[nx], ground_f[n_feet 3], anchors[n_feet 3].
// Prints the recorded rows, then the metrics (steps, first_nonfinite, first_out, n_not_solved,
// n_ls_rejected, max_dz, min_cz, max_viol), then seen, recorded, dropped: one value per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "record.h"

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
  const int nx = hd[0], nu0 = hd[1], nfeet = hd[2], qoff = hd[3], capacity = hd[4], every = hd[5], steps = hd[6];
  double tol[3];
  rd(f, tol, sizeof(tol));
  const double never = 1.7976931348623157e308;
  const double dz_tol = (hd[7] & 1) ? tol[1] : never, cz_min = (hd[7] & 2) ? tol[2] : -never;
  const pl::RecLayout L = pl::rec_layout(nx, nu0, nfeet);
  // on the heap, exactly sized: the sanitizer sees every access past an end
  std::vector<double> log((size_t)capacity * L.row);
  std::vector<PlMpcMetrics> met(1);
  pl::rec_metrics_reset(met[0]);
  std::vector<long long> cur(3, 0);
  for (int s = 0; s < steps; ++s) {
    std::vector<double> k(1), xi(nx), u0(nu0), st(8), xs(nx), gf(3 * nfeet), an(3 * nfeet);
    rd(f, k.data(), 8);
    rd(f, xi.data(), nx * 8);
    rd(f, u0.data(), nu0 * 8);
    rd(f, st.data(), 8 * 8);
    rd(f, xs.data(), nx * 8);
    rd(f, gf.data(), 3 * nfeet * 8);
    rd(f, an.data(), 3 * nfeet * 8);
    std::vector<PlProbInfo> info(1);
    memset(info.data(), 0, sizeof(PlProbInfo));
    info[0].status = (int)st[0];
    info[0].iter = (int)st[1];
    info[0].ls_accepted = (int)st[2];
    info[0].ls_alpha = st[3];
    info[0].viol_max = st[4];
    info[0].f = st[5];
    info[0].pri_res = st[6];
    info[0].dua_res = st[7];
    const pl::RecSrc S{xi.data(), u0.data(), info.data(), xs.data(), gf.data(), an.data()};
    pl::record_host(nx, nu0, nfeet, qoff, (int)k[0], S, tol[0], dz_tol, cz_min, capacity, every, cur.data(),
                    log.empty() ? nullptr : log.data(), met.data());
  }
  fclose(f);
  for (size_t e = 0; e < (size_t)cur[1] * L.row; ++e) printf("%.17g\n", log[e]);
  const PlMpcMetrics& m = met[0];
  printf("%d\n%d\n%d\n%d\n%d\n%.17g\n%.17g\n%.17g\n", m.steps, m.first_nonfinite, m.first_out, m.n_not_solved,
         m.n_ls_rejected, m.max_dz, m.min_cz, m.max_viol);
  printf("%lld\n%lld\n%lld\n", cur[0], cur[1], cur[2]);
  return 0;
}
