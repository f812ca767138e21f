// TEST INFRASTRUCTURE: a stand-alone host program around pl::timeline_prepare_host
// (csrc/timeline.h), the body of pl_mpc_timeline_host and the code k_mpc_prepare runs with a
// timeline, so that the CPU suite can run it under AddressSanitizer / UBSan directly, with nothing
// loaded into python (tests/test_timeline_host.py).  Not linked into the product.
//
// Input file (argv[1]), native byte order: int32 N, nf, dyn, na, ndx, ext_valid, arm_valid, np, n,
// count, steps; int32 parameter offsets x_init, dt_min, dt_max, contact, swing, n_contacts,
// swing_period, base_vel_des, ext_force_des, arm_vel_des; int32 x_off[N]; doubles total_mass, t0;
// `count` keyframes of 128 bytes (pl_mpc_keyframe); doubles p[np], x[n]; int32 k[steps].
// The keyframes sit in a heap block of exactly count entries, p and x in blocks of exactly np and
// n doubles: a read past a problem's count, or a write outside p or x, is a sanitizer report.
// Prints per step: seg, gait_type, then p[np] and x[n], one value per line; every step starts
// from the p and x of the file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "timeline.h"

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
  int hd[11], po[10];
  rd(f, hd, sizeof(hd));
  rd(f, po, sizeof(po));
  const int N = hd[0], np = hd[7], n = hd[8], count = hd[9], steps = hd[10];
  std::vector<PlOcpConst> Ov(1);
  std::vector<PlModel> Mv(1);
  memset(Ov.data(), 0, sizeof(PlOcpConst));
  memset(Mv.data(), 0, sizeof(PlModel));
  PlOcpConst& O = Ov[0];
  O.N = N;
  O.nf = hd[1];
  O.dyn = hd[2];
  O.na = hd[3];
  O.ndx = hd[4];
  O.ext.valid = hd[5];
  O.arm.valid = hd[6];
  O.nfeet = 4;
  O.P.x_init = po[0];
  O.P.dt_min = po[1];
  O.P.dt_max = po[2];
  O.P.contact = po[3];
  O.P.swing = po[4];
  O.P.n_contacts = po[5];
  O.P.swing_period = po[6];
  O.P.base_vel_des = po[7];
  O.P.ext_force_des = po[8];
  O.P.arm_vel_des = po[9];
  O.P.np = np;
  std::vector<int> xoff(N);
  rd(f, xoff.data(), N * sizeof(int));
  std::vector<PlNode> nodes(N);
  memset(nodes.data(), 0, N * sizeof(PlNode));
  for (int i = 0; i < N; ++i) nodes[i].x_off = xoff[i];
  double sc[2];
  rd(f, sc, sizeof(sc));
  Mv[0].total_mass = sc[0];
  const double t0 = sc[1];
  std::vector<PlKeyframe> keys(count);
  rd(f, keys.data(), (size_t)count * sizeof(PlKeyframe));
  std::vector<double> p0(np), x0(n);
  rd(f, p0.data(), (size_t)np * 8);
  rd(f, x0.data(), (size_t)n * 8);
  std::vector<int> ks(steps);
  rd(f, ks.data(), steps * sizeof(int));
  fclose(f);
  for (int s = 0; s < steps; ++s) {
    std::vector<double> p(p0), x(x0);
    std::vector<PlTimelineState> st(1);
    pl::timeline_prepare_host(Mv[0], O, nodes.data(), ks[s], t0, keys.data(), count, p.data(), x.data(), st.data());
    printf("%d\n%d\n", st[0].seg, st[0].gait_type);
    for (int j = 0; j < np; ++j) printf("%.17g\n", p[j]);
    for (int j = 0; j < n; ++j) printf("%.17g\n", x[j]);
  }
  return 0;
}
