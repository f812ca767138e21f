// C-ABI, profiling and test hooks (include/pinoloco.h): stream sync, the per-launch event
// timing, the size report and the pl_debug_* access to internal arrays and single stages.
#include "api_internal.h"

void prof_collect(PlOcpHandle* h) {
  if (!h->profile || (h->prof_n == 0 && h->prof_hn == 0)) return;
  hipStreamSynchronize(h->stream);
  for (int k = 0; k < h->prof_hn; ++k) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->prof_hev[k][0], h->prof_hev[k][1]);
    h->prof_hess_ms += ms;
    h->prof_hess_launches++;
  }
  h->prof_hn = 0;
  for (int k = 0; k < h->prof_n; ++k) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->prof_ev[k][0], h->prof_ev[k][1]);
    h->prof_admm_ms += ms;
    h->prof_admm_launches++;
  }
  h->prof_n = 0;
}

extern "C" int pl_ocp_sync(pl_ocp* o) {
  REQUIRE_DEVICE(o);
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  prof_collect(&o->h);
  return 0;
}

// Per-launch timing of the dominant kernel (k_admm) with HIP events recorded on
// the handle's stream around every launch.  enable=1 starts (and clears),
// enable=0 stops.  out: [total_ms, launches, problem_iterations].
extern "C" int pl_ocp_profile(pl_ocp* o, int enable) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  prof_collect(h);
  if (enable && !h->profile) {
    for (int k = 0; k < 64; ++k) {
      hipEventCreate(&h->prof_ev[k][0]);
      hipEventCreate(&h->prof_ev[k][1]);
    }
    for (int k = 0; k < 16; ++k) {
      hipEventCreate(&h->prof_hev[k][0]);
      hipEventCreate(&h->prof_hev[k][1]);
    }
  }
  h->profile = enable;
  h->prof_n = 0;
  h->prof_admm_ms = 0.0;
  h->prof_admm_launches = 0;
  h->prof_admm_iters = 0;
  h->prof_hn = 0;
  h->prof_hess_ms = 0.0;
  h->prof_hess_launches = 0;
  if (enable && h->d.ip_act) PL_CHECK_HIP(hipMemsetAsync(h->d.ip_act + h->B + 1, 0, sizeof(int), h->stream));
  if (enable) {
    launch_reset_prof(h);
    PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int pl_ocp_profile_read(pl_ocp* o, double* out) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  prof_collect(h);
  // problem-iterations the ADMM launches actually executed: per-problem counters
  // (terminated problems skip later launches, so B * niter would over-count)
  std::vector<PlProbInfo> info(h->B);
  PL_CHECK_HIP(hipMemcpyAsync(info.data(), h->d.info, h->B * sizeof(PlProbInfo), hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  long long it = 0;
  for (int b = 0; b < h->B; ++b) it += info[b].iter_prof;
  h->prof_admm_iters = it;
  out[0] = h->prof_admm_ms;
  out[1] = (double)h->prof_admm_launches;
  out[2] = (double)h->prof_admm_iters;
  return 0;
}

// Per-launch timing of the interior point's Lagrangian Hessian (k_lag_hess), recorded with the
// ADMM timing while pl_ocp_profile is on.  out: [total_ms, launches].
extern "C" int pl_ocp_profile_read_hess(pl_ocp* o, double* out) {
  REQUIRE_DEVICE(o);
  if (!out) { pl_set_error("null argument"); return -1; }
  prof_collect(&o->h);
  out[0] = o->h.prof_hess_ms;
  out[1] = (double)o->h.prof_hess_launches;
  int lanes = 0;  // Hessian lanes launched since profiling started (k_ip_compact)
  if (o->h.d.ip_act)
    PL_CHECK_HIP(hipMemcpy(&lanes, o->h.d.ip_act + o->h.B + 1, sizeof(int), hipMemcpyDeviceToHost));
  out[2] = o->h.prof_hess_launches > 0 ? (double)lanes / o->h.prof_hess_launches : 0.0;
  return 0;
}

int admm_lds_bytes(const PlOcpHandle* h);
int admm_ppw(const PlOcpHandle* h);
int admm_asb_cap(const PlOcpHandle* h);

// Sizes: [n, m, nnz, S_stride (doubles), nw_max, N, ADMM programs (u16, LDS-resident),
// problems per ADMM workgroup, ADMM LDS bytes per workgroup, A values per lane / 64,
// A values per problem staged in LDS by the one-wave sweep, largest node's A count].
extern "C" int pl_ocp_sizes(const pl_ocp* o, long long* out) {
  if (!o) { pl_set_error("null handle"); return -1; }
  out[0] = o->h.n; out[1] = o->h.m; out[2] = o->h.nnz; out[3] = o->h.S_stride; out[4] = o->h.nw_max; out[5] = o->h.N;
  out[6] = (long long)o->aprog.size(); out[7] = admm_ppw(&o->h); out[8] = admm_lds_bytes(&o->h); out[9] = o->h.admm_asr;
  out[10] = admm_asb_cap(&o->h); out[11] = o->h.nent_max; out[12] = o->h.debug_paths;
  return 0;
}

// The arrays that are not doubles on the device, passed as doubles (interior-point stage tests):
// "ip_iflag" [B][4], "info_done" [B] (PlProbInfo::done) and "ipinfo" [B][PL_IPINFO_DOUBLES] in
// the field order of include/pinoloco.h.  1: handled, 0: another name, < 0: error.
static int debug_rw_records(pl_ocp* o, const char* name, double* out, const double* in, long long count) {
  PlOcpHandle* h = &o->h;
  const size_t B = h->B;
  const int which = !strcmp(name, "ip_iflag") ? 0 : !strcmp(name, "info_done") ? 1 : !strcmp(name, "ipinfo") ? 2 : -1;
  if (which < 0) return 0;
  if (which != 1 && !h->d.ipinfo) { pl_set_error("array %s not allocated (set_solver first)", name); return -1; }
  const size_t len = B * (which == 0 ? 4 : which == 1 ? 1 : PL_IPINFO_DOUBLES);
  if ((size_t)count < len) { pl_set_error("buffer too small for %s (%zu)", name, len); return -1; }
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  if (which == 0) {
    std::vector<int> F(4 * B);
    if (out) {
      PL_CHECK_HIP(hipMemcpy(F.data(), h->d.ip_iflag, F.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (size_t q = 0; q < F.size(); ++q) out[q] = F[q];
    } else {
      for (size_t q = 0; q < F.size(); ++q) F[q] = (int)in[q];
      PL_CHECK_HIP(hipMemcpy(h->d.ip_iflag, F.data(), F.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return 1;
  }
  if (which == 1) {
    std::vector<PlProbInfo> info(B);
    PL_CHECK_HIP(hipMemcpy(info.data(), h->d.info, B * sizeof(PlProbInfo), hipMemcpyDeviceToHost));
    if (out) {
      for (size_t b = 0; b < B; ++b) out[b] = info[b].done;
    } else {
      for (size_t b = 0; b < B; ++b) info[b].done = (int)in[b];
      PL_CHECK_HIP(hipMemcpy(h->d.info, info.data(), B * sizeof(PlProbInfo), hipMemcpyHostToDevice));
    }
    return 1;
  }
  static_assert(PL_IPINFO_DOUBLES == 15 + 3 * PL_IP_MAXFILT, "ipinfo record (include/pinoloco.h)");
  std::vector<PlIpInfo> ip(B);
  PL_CHECK_HIP(hipMemcpy(ip.data(), h->d.ipinfo, B * sizeof(PlIpInfo), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; ++b) {
    PlIpInfo& s = ip[b];
    if (out) {
      double* r = out + b * PL_IPINFO_DOUBLES;
      const double head[15] = {s.mu, s.theta_max, s.theta_min, s.err, s.f, s.alpha, s.alpha_z, s.viol_max,
                               (double)s.iter, (double)s.status, (double)s.nfilt, (double)s.trials,
                               (double)s.active, (double)s.ref_solves, s.ref_last};
      for (int q = 0; q < 15; ++q) r[q] = head[q];
      for (int q = 0; q < 2 * PL_IP_MAXFILT; ++q) r[15 + q] = s.filt[q];
      for (int q = 0; q < PL_IP_MAXFILT; ++q) r[15 + 2 * PL_IP_MAXFILT + q] = s.alphas[q];
    } else {
      const double* r = in + b * PL_IPINFO_DOUBLES;
      s.mu = r[0]; s.theta_max = r[1]; s.theta_min = r[2]; s.err = r[3]; s.f = r[4]; s.alpha = r[5];
      s.alpha_z = r[6]; s.viol_max = r[7];
      s.iter = (int)r[8]; s.status = (int)r[9]; s.nfilt = (int)r[10]; s.trials = (int)r[11];
      s.active = (int)r[12]; s.ref_solves = (int)r[13]; s.ref_last = r[14];
      if (s.iter < 0 || s.iter >= PL_IP_MAXFILT || s.nfilt < 0 || s.nfilt > PL_IP_MAXFILT) {
        pl_set_error("ipinfo: iter %d or nfilt %d outside the record", s.iter, s.nfilt);
        return -1;
      }
      for (int q = 0; q < 2 * PL_IP_MAXFILT; ++q) s.filt[q] = r[15 + q];
      for (int q = 0; q < PL_IP_MAXFILT; ++q) s.alphas[q] = r[15 + 2 * PL_IP_MAXFILT + q];
    }
  }
  if (in) PL_CHECK_HIP(hipMemcpy(h->d.ipinfo, ip.data(), B * sizeof(PlIpInfo), hipMemcpyHostToDevice));
  return 1;
}

// Debug / parity access to internal per-problem arrays (tests only).
static int debug_rw(pl_ocp* o, const char* name, double* out, const double* in, long long count) {
  PlOcpHandle* h = &o->h;
  const size_t B = h->B;
  if (const int rec = debug_rw_records(o, name, out, in, count)) return rec < 0 ? rec : 0;
  struct Item { const char* n; double* p; size_t len; } items[] = {
      {"Hlag", h->d.Hlag, h->d.Hlag ? B * (size_t)h->hl_stride : 0},
      {"ip_dwi", h->d.ip_dwi, h->d.ip_dwi ? 2 * B : 0}, {"work", h->d.work, B * 8},
      {"As", h->d.As, B * h->nnz}, {"Araw", h->d.Araw, B * h->nnz}, {"qs", h->d.qs, B * h->n},
      {"ls", h->d.ls, B * h->m},   {"us", h->d.us, B * h->m},       {"rho", h->d.rho, B * h->m},
      {"D", h->d.D, B * h->n},     {"E", h->d.E, B * h->m},         {"cs", h->d.cs, B},
      {"admm_t", h->d.dbg, h->d.dbg ? B * 40 : 0}, {"Ps", h->d.Ps, B * h->n},   {"P", h->d.P, B * h->n},         {"xa", h->d.xa, B * h->n},
      {"za", h->d.za, B * h->m},   {"ya", h->d.ya, B * h->m},       {"S", h->d.S, B * (size_t)h->S_stride},
      {"FS", h->d.FS, h->d.FS ? B * (size_t)h->fs_stride : 0},
      {"rhs", h->d.rhs, B * h->n}, {"step", h->d.step, B * h->n},   {"grad", h->d.grad, B * h->n},
      {"g", h->d.g, B * h->m},     {"xstate", h->d.xstate, B * h->nx},
      {"dxs", h->d.dxs, B * h->n}, {"dys", h->d.dys, B * h->m},     {"chk", h->d.chk, B * (size_t)(h->N + 1) * 8},
      {"lbg", h->d.lbg, B * h->m}, {"ubg", h->d.ubg, B * h->m},
      {"rhoc", h->d.rhoc, B * (size_t)(h->N + 1) * std::max(h->ncpl_max, 1)},
      {"rho_upd_it", h->ra.upd_it, h->ra.upd_it ? B * PL_RHO_LOG : 0},
      {"ip_s", h->d.ip_s, h->d.ip_s ? B * h->m : 0},     {"ip_lam", h->d.ip_lam, h->d.ip_lam ? B * h->m : 0},
      {"ip_lam0", h->d.ip_lam0, h->d.ip_lam0 ? B * h->m : 0},
      {"ip_zl", h->d.ip_zl, h->d.ip_zl ? B * h->m : 0},  {"ip_zu", h->d.ip_zu, h->d.ip_zu ? B * h->m : 0},
      {"ip_rh", h->d.ip_rh, h->d.ip_rh ? B * h->m : 0},  {"ip_dl", h->d.ip_dl, h->d.ip_dl ? B * h->m : 0},
      {"ip_ds", h->d.ip_ds, h->d.ip_ds ? B * h->m : 0},  {"ip_dx", h->d.ip_dx, h->d.ip_dx ? B * h->n : 0},
      {"ip_jdx", h->d.ip_jdx, h->d.ip_jdx ? B * h->m : 0}};
  for (auto& it : items) {
    if (strcmp(it.n, name) == 0) {
      if (!it.p) { pl_set_error("array %s not allocated (set_solver first)", name); return -1; }
      if ((size_t)count < it.len) { pl_set_error("buffer too small for %s (%zu)", name, it.len); return -1; }
      if (out) PL_CHECK_HIP(hipMemcpyAsync(out, it.p, it.len * 8, hipMemcpyDeviceToHost, h->stream));
      else PL_CHECK_HIP(hipMemcpyAsync(it.p, in, it.len * 8, hipMemcpyHostToDevice, h->stream));
      if (in && it.p == h->d.Araw) {  // the constant entries are rewritten by the next (eager) step
        h->jac_cheap_ok = 0;
        o->mpc_key.clear();
      }
      if (in && it.p == h->d.rho) {  // no longer k_qp_finish's values: the sweep streams them
        h->admm_rho_rule = 0;
        o->mpc_key.clear();
      }
      PL_CHECK_HIP(hipStreamSynchronize(h->stream));
      return (int)0;
    }
  }
  pl_set_error("unknown array %s", name);
  return -1;
}

extern "C" int pl_debug_get(pl_ocp* o, const char* name, double* out, long long count) {
  REQUIRE_DEVICE(o);
  if (!out) { pl_set_error("null argument"); return -1; }
  return debug_rw(o, name, out, nullptr, count);
}

// Overwrite an internal array (tests: e.g. "ip_dwi", the inertia state of a teacher-forced
// interior-point direction).
extern "C" int pl_debug_set(pl_ocp* o, const char* name, const double* in, long long count) {
  REQUIRE_DEVICE(o);
  if (!in) { pl_set_error("null argument"); return -1; }
  return debug_rw(o, name, nullptr, in, count);
}

// Node table (tests): per node [nw, nu, x_off, row_off, nrow, ncol, ent_off, nent, ntile, nunit, s_off, ncpl]
extern "C" int pl_debug_nodes(const pl_ocp* o, int* out) {
  for (size_t i = 0; i < o->nodes.size(); ++i) {
    const PlNode& nd = o->nodes[i];
    int* r = out + 12 * i;
    r[0] = nd.nw; r[1] = nd.nu; r[2] = nd.x_off; r[3] = nd.row_off; r[4] = nd.nrow; r[5] = nd.ncol;
    r[6] = nd.ent_off; r[7] = nd.nent; r[8] = nd.ntile; r[9] = nd.nunit; r[10] = nd.s_off; r[11] = nd.ncpl;
  }
  return 0;
}

// Raw copies of the host-built descriptors (tests: host build of the device math).
extern "C" int pl_debug_consts(const pl_ocp* o, void* model_out, void* oc_out, int* sizes) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (sizes) { sizes[0] = (int)sizeof(PlModel); sizes[1] = (int)sizeof(PlOcpConst); }
  if (model_out) memcpy(model_out, &o->h.model, sizeof(PlModel));
  if (oc_out) memcpy(oc_out, &o->h.oc, sizeof(PlOcpConst));
  return 0;
}

// Tests: evaluate + scale + factor, then exactly `niter` ADMM iterations from the
// current iterates (no termination checks, no line search).  reset bit 0: from x = z = y = 0;
// bit 1: the last iteration stores delta x / delta y (d.dxs, d.dys) as a check iteration of
// pl_ocp_solve does.
extern "C" int pl_debug_admm(pl_ocp* o, int niter, int reset) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_eval_values(h, h->d.x);
  launch_eval_jac(h);
  launch_objective(h);
  launch_qp_setup(h);
  launch_factor(h);
  launch_reset_info(h);
  if (reset & 1) launch_reset_iterates(h);
  launch_admm_init(h);
  if (niter > 0) launch_admm(h, niter, (reset & 2) ? 1 : 0, 0);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Tests: Ruiz scaling and k_qp_finish alone on whatever Araw, P, grad, g, lbg, ubg hold now
// (no evaluation, so pl_debug_set can overwrite the raw data first; no factor).
extern "C" int pl_debug_qp_setup(pl_ocp* o) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_qp_setup(h);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Tests: one termination check (k_check_part, k_check) on the current xa, za, ya, dxs, dys
// and scaled data, then k_unscale if asked; status, pri_res and dua_res come back through
// pl_mpc_get_stats.  Does not evaluate, scale or factor.
extern "C" int pl_debug_check(pl_ocp* o, int final_check, int unscale) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_reset_info(h);
  launch_check(h, 0, final_check ? 1 : 0);
  if (unscale) launch_unscale(h);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// Tests: the device's raw Philox blocks (noise.h, k_rng_blocks) for the seeds pl_mpc_set_noise
// holds: block i of problem b at the counter (k, i0 + i, stream, c3); the loop's draws have
// i0 = c3 = 0.  The integer part of the generator, away from any libm.
extern "C" int pl_debug_rng(pl_ocp* o, unsigned k, unsigned stream, unsigned i0, unsigned c3, int n_blocks,
                            unsigned* out) {
  if (!o || !out) { pl_set_error("pl_debug_rng: null argument"); return -1; }
  if (n_blocks < 1 || n_blocks > 65536) { pl_set_error("pl_debug_rng: n_blocks %d outside [1, 65536]", n_blocks); return -1; }
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->rng_seed) { pl_set_error("pl_debug_rng: no seeds were given (pl_mpc_set_noise)"); return -1; }
  const size_t words = (size_t)h->B * n_blocks * 4;
  unsigned* dev = nullptr;
  PL_CHECK_HIP(hipMalloc((void**)&dev, words * sizeof(unsigned)));
  launch_rng_blocks(h, k, stream, i0, c3, n_blocks, dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, dev, words * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(dev);
  PL_CHECK_HIP(e);
  return 0;
}
