// C-ABI, device MPC loop (include/pinoloco.h): setup, the plant and its disturbances and
// contact, the step with its graph capture and replay, state / stats / export / download, the
// rollout log with its metrics and push schedule, and the gait and command timelines.
#include "api_internal.h"
#include "noise.h"
#include "plant.h"
#include "record.h"
#include "timeline.h"

extern "C" int pl_mpc_setup(pl_ocp* o, const double* x_state, const double* t0) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  PL_CHECK_HIP(hipMemcpyAsync(h->d.xstate, x_state, (size_t)h->B * h->nx * 8, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->d.t0, t0, (size_t)h->B * 8, hipMemcpyHostToDevice, h->stream));
  // a new loop: no foot has touched down yet (the contact plant's anchors and last forces)
  const size_t cb = (size_t)h->B * h->oc.nfeet * 3 * 8;
  PL_CHECK_HIP(hipMemsetAsync(h->d.plant_anchor, 0, cb, h->stream));
  PL_CHECK_HIP(hipMemsetAsync(h->d.plant_cf, 0, cb, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  h->ip_lam_warm = 0;  // the loop's first solve has no lam_g yet (ocp.py:198)
  return 0;
}

// ---------------------------------------------------------------------------
// The plant of the loop: what turns the solve of step k into the true state of step k + 1.
// PL_PLANT_NOMINAL is the reference's own loop, the optimiser's prediction (run_mpc.py:142);
// PL_PLANT_ABA steps the forward dynamics under the commanded torques and forces and a base
// wrench (plant.h, k_plant.hip).  The settings are host state inside the MPC graph key; the
// disturbance values are device data the launches read, so new values replay.
extern "C" int pl_mpc_set_plant(pl_ocp* o, int mode, int substeps) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (mode != PL_PLANT_NOMINAL && mode != PL_PLANT_ABA) { pl_set_error("pl_mpc_set_plant: unknown mode %d", mode); return -1; }
  if (substeps < 1 || substeps > 16) { pl_set_error("pl_mpc_set_plant: substeps %d outside [1, 16]", substeps); return -1; }
  if (mode == PL_PLANT_ABA && PL_IS_CV(o->h.oc.dyn)) {
    pl_set_error("pl_mpc_set_plant: PL_PLANT_ABA is defined on x = [q, v]; centroidal_vel has x = [h, q]");
    return -1;
  }
  o->h.plant_mode = mode;
  o->h.plant_substeps = substeps;
  return 0;
}

extern "C" int pl_mpc_get_plant(const pl_ocp* o, int* mode, int* substeps) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (mode) *mode = o->h.plant_mode;
  if (substeps) *substeps = o->h.plant_substeps;
  return 0;
}

extern "C" int pl_mpc_set_disturbance(pl_ocp* o, const double* base_wrench, const double* state_noise) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (base_wrench && h->push_on) {  // one owner of d.plant_w
    pl_set_error("pl_mpc_set_disturbance: a push schedule is set (pl_mpc_set_push) and owns the base wrench");
    return -1;
  }
  if (base_wrench && h->rng_wrench_on) {
    pl_set_error("pl_mpc_set_disturbance: a random base wrench is set (pl_mpc_set_noise) and owns the base wrench");
    return -1;
  }
  if (state_noise && h->rng_state_on) {  // one owner of d.plant_noise
    pl_set_error("pl_mpc_set_disturbance: a random state noise is set (pl_mpc_set_noise) and owns the state noise");
    return -1;
  }
  const size_t wb = (size_t)h->B * 6 * 8, nb = (size_t)h->B * h->ndx * 8;
  if (base_wrench) PL_CHECK_HIP(hipMemcpyAsync(h->d.plant_w, base_wrench, wb, hipMemcpyHostToDevice, h->stream));
  else if (!h->push_on && !h->rng_wrench_on)  // k_plant always reads it: zero = none
    PL_CHECK_HIP(hipMemsetAsync(h->d.plant_w, 0, wb, h->stream));
  if (state_noise) PL_CHECK_HIP(hipMemcpyAsync(h->d.plant_noise, state_noise, nb, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  h->plant_noise_on = state_noise ? 1 : 0;  // off: k_mpc_prepare's plain copy of x_state
  h->dist_wrench_on = base_wrench ? 1 : 0;
  return 0;
}

// Ground contact at the feet and the joint PD loop of PL_PLANT_ABA (plant.h).  The switch is
// host state inside the graph key; parameters, ground heights, anchors and last forces are
// device data, so new values replay.
static_assert(sizeof(pl_contact_params) == sizeof(PlContact), "pl_contact_params and PlContact are one layout");

static int contact_check(const char* who, const pl_ocp* o, const pl_contact_params* prm, int count) {
  if (PL_IS_CV(o->h.oc.dyn)) {
    pl_set_error("%s: the contact plant is defined on x = [q, v]; centroidal_vel has x = [h, q]", who);
    return -1;
  }
  static const char* const names[7] = {"k_n", "d_n", "k_t", "d_t", "mu", "kp", "kd"};
  for (int b = 0; prm && b < count; ++b) {
    const double* f = &prm[b].k_n;
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(f[k]) || f[k] < 0.0) {
        pl_set_error("%s: problem %d: %s = %g is negative or not finite", who, b, names[k], f[k]);
        return -1;
      }
    if (!(prm[b].k_n > 0.0)) {
      pl_set_error("%s: problem %d: k_n = %g must be positive", who, b, prm[b].k_n);
      return -1;
    }
  }
  return 0;
}

extern "C" int pl_mpc_set_contact(pl_ocp* o, const pl_contact_params* prm, const double* ground_z) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (contact_check("pl_mpc_set_contact", o, prm, o->h.B)) return -1;
  if (prm && !ground_z) { pl_set_error("pl_mpc_set_contact: ground_z is null"); return -1; }
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (prm) {
    PL_CHECK_HIP(hipMemcpyAsync(h->d.plant_cprm, prm, (size_t)h->B * sizeof(PlContact), hipMemcpyHostToDevice, h->stream));
    PL_CHECK_HIP(hipMemcpyAsync(h->d.plant_gz, ground_z, (size_t)h->B * h->oc.nfeet * 8, hipMemcpyHostToDevice, h->stream));
    PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  }
  h->plant_contact_on = prm ? 1 : 0;
  return 0;
}

extern "C" int pl_mpc_get_contact(pl_ocp* o, int* on, double* anchors, double* forces) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  const size_t cb = (size_t)h->B * h->oc.nfeet * 3 * 8;
  if (on) *on = h->plant_contact_on;
  if (anchors) PL_CHECK_HIP(hipMemcpyAsync(anchors, h->d.plant_anchor, cb, hipMemcpyDeviceToHost, h->stream));
  if (forces) PL_CHECK_HIP(hipMemcpyAsync(forces, h->d.plant_cf, cb, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_mpc_plant_host(const pl_ocp* o, const double* p, const double* x, const double* base_wrench,
                                 const pl_contact_params* prm, const double* ground_z, double* anchors, int substeps,
                                 double* x_state, double* forces) {
  if (!o || !p || !x || !x_state) { pl_set_error("pl_mpc_plant_host: null argument"); return -1; }
  if (substeps < 1 || substeps > 16) { pl_set_error("pl_mpc_plant_host: substeps %d outside [1, 16]", substeps); return -1; }
  if (contact_check("pl_mpc_plant_host", o, prm, 1)) return -1;
  if (prm && (!ground_z || !anchors)) { pl_set_error("pl_mpc_plant_host: contact needs ground_z and anchors"); return -1; }
  const PlOcpHandle& h = o->h;
  if (!prm) {
    pl::plant_step<false>(h.model, h.oc, h.oc.dyn, o->nodes.data(), h.N, p, x, base_wrench, substeps, x_state);
    return 0;
  }
  double fg[3 * PL_MAXFEET] = {0.0};
  PlContact c;
  memcpy(&c, prm, sizeof(c));
  pl::plant_step<true>(h.model, h.oc, h.oc.dyn, o->nodes.data(), h.N, p, x, base_wrench, substeps, x_state, &c, ground_z,
                       anchors, fg);
  if (forces)
    for (int k = 0; k < 3 * h.oc.nfeet; ++k) forces[k] = fg[k];
  return 0;
}

static void enqueue_mpc_plant(PlOcpHandle* h) {
  if (h->plant_mode == PL_PLANT_ABA) launch_plant(h);
  else launch_mpc_finish(h);
}

// The OSQP-SQP part of an MPC step (every launch after k_mpc_prepare) as one HIP graph.
// The sequence is fixed by the handle's host state (sizes, settings, kernel choice,
// device pointers): it is captured on the second step that sees the same bytes of `h`
// (the first runs eagerly, so every one-time kernel attribute is set outside a capture)
// and replayed while they stay the same; any change (a setter, another kernel choice)
// runs eagerly once and re-captures.  Per-call data lives in device memory, so a replay
// is the eager sequence.  Profiling runs (per-launch events) and PL_MPC_GRAPH=0 stay eager.
static void enqueue_mpc_sqp(pl_ocp* o) {
  for (int it = 0; it < o->h.sqp_iters; ++it) enqueue_solve(o, false);
  enqueue_mpc_plant(&o->h);
}

// The key is the handle up to its profiling fields: every launcher takes its launch
// parameters (grid, LDS bytes, kernel choice, pointers, settings) from `h` and from
// nothing else (no getenv, statics or pl_ocp fields at launch time), so equal bytes mean
// an equal launch sequence.  Profiling runs never replay (pl_mpc_step), so the event
// handles and counters stay out of the key.
static constexpr size_t kMpcKeyBytes = offsetof(PlOcpHandle, profile);

static int mpc_sqp_graph(pl_ocp* o) {
  PlOcpHandle* h = &o->h;
  const unsigned char* hb = reinterpret_cast<const unsigned char*>(h);
  const bool same = o->mpc_key.size() == kMpcKeyBytes && !memcmp(o->mpc_key.data(), hb, kMpcKeyBytes);
  if (same && o->mpc_graph) {
    ++o->mpc_replays;
    return hipGraphLaunch(o->mpc_graph, h->stream) == hipSuccess ? 0 : -1;
  }
  if (o->mpc_graph) {
    hipGraphExecDestroy(o->mpc_graph);
    o->mpc_graph = nullptr;
  }
  if (!same) {  // first sighting of this state: eager, remember it
    o->mpc_key.assign(hb, hb + kMpcKeyBytes);
    enqueue_mpc_sqp(o);
    return 0;
  }
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return -1;
  enqueue_mpc_sqp(o);
  const hipError_t ec = hipStreamEndCapture(h->stream, &g);
  if (ec != hipSuccess || !g) {
    (void)hipGetLastError();
    if (g) hipGraphDestroy(g);
    return -1;
  }
  const hipError_t ei = hipGraphInstantiate(&o->mpc_graph, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (ei != hipSuccess) {
    o->mpc_graph = nullptr;
    return -1;
  }
  ++o->mpc_captures;
  ++o->mpc_replays;
  return hipGraphLaunch(o->mpc_graph, h->stream) == hipSuccess ? 0 : -1;
}

extern "C" int pl_mpc_set_ip_lam(pl_ocp* o, int carry) {
  if (!o || (carry != 0 && carry != 1)) { pl_set_error("pl_mpc_set_ip_lam: carry must be 0 or 1"); return -1; }
  o->h.ip_mpc_lam = carry;
  return 0;
}

// MPC-step graph state (tests): [captures, replays, eager fallback (1: capture or replay
// failed, or PL_MPC_GRAPH=0)].
extern "C" int pl_mpc_graph_info(const pl_ocp* o, long long* out) {
  if (!o || !out) { pl_set_error("null argument"); return -1; }
  out[0] = o->mpc_captures;
  out[1] = o->mpc_replays;
  out[2] = o->mpc_graph_off;
  return 0;
}

static int mpc_step_sequence(pl_ocp* o, int k) {
  // the event slots: 64 ADMM launches, 16 Hessian launches (an interior-point step makes <= 10)
  if (o->h.profile && (o->h.prof_n > 48 || o->h.prof_hn > 0)) prof_collect(&o->h);
  launch_mpc_prepare(&o->h, k);
  if (o->h.solver != PL_SOLVER_IP && !o->h.profile && !o->mpc_graph_off) {
    if (mpc_sqp_graph(o)) {
      // capture or replay refused: nothing of the step ran; from now on launch eagerly
      (void)hipGetLastError();
      o->mpc_graph_off = 1;
      enqueue_mpc_sqp(o);
    }
    PL_CHECK_HIP(hipGetLastError());
    return 0;
  }
  if (o->h.solver == PL_SOLVER_IP) {
    enqueue_ip(&o->h);
    PlOcpHandle* h = &o->h;
    if (h->ip_mpc_lam) {
      // the Opti branch (compile_solver = False): warm_start() of the next step passes this
      // solve's lam_g back (ocp.py:373, ocp_*.py warm_start)
      PL_CHECK_HIP(hipMemcpyAsync(h->d.ip_lam0, h->d.ip_lam, (size_t)h->B * h->m * 8, hipMemcpyDeviceToDevice,
                                  h->stream));
      h->ip_lam_warm = 1;
    } else {
      // the reference's default driver (solver "fatrop", compile_solver = True, run_mpc.py:34-37,
      // 50-111): the compiled solver takes the primal warm start only (its inputs end with opti.x,
      // ocp_whole_body_rnea.py:239-257, the lam_g output commented out), so every solve starts
      // from cold multipliers
      h->ip_lam_warm = 0;
    }
    enqueue_mpc_plant(&o->h);
  } else
    enqueue_mpc_sqp(o);
  PL_CHECK_HIP(hipGetLastError());
  return 0;
}

// The step's sequence, then, while the log is on, its record launch (k_record.hip): outside the
// captured step, with the step index and the slot as plain arguments.
extern "C" int pl_mpc_step(pl_ocp* o, int k) {
  REQUIRE_DEVICE(o);
  const int rc = mpc_step_sequence(o, k);
  if (rc) return rc;
  PlOcpHandle* h = &o->h;
  if (h->rec_on) {
    launch_mpc_record(h, k, pl::rec_slot(h->rec_capacity, h->rec_every, h->rec_cur), o->nodes[0].nu);
    PL_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int pl_mpc_run(pl_ocp* o, int k0, int steps) {
  REQUIRE_DEVICE(o);
  if (steps < 0) { pl_set_error("pl_mpc_run: steps %d is negative", steps); return -1; }
  for (int k = k0; k < k0 + steps; ++k) {
    const int rc = pl_mpc_step(o, k);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int pl_mpc_get_state(pl_ocp* o, double* x_state) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  PL_CHECK_HIP(hipMemcpyAsync(x_state, h->d.xstate, (size_t)h->B * h->nx * 8, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_mpc_get_stats(pl_ocp* o, pl_stats* stats) {
  REQUIRE_DEVICE(o);
  return fetch_stats(o, stats);
}

extern "C" int pl_mpc_export(pl_ocp* o, void* device_dst) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  const int nu0 = o->nodes[0].nu;
  const size_t row = (size_t)nu0 + h->nx;
  char* dst = (char*)device_dst;
  // two strided copies on the handle's stream: u_0 of every problem, then x_state
  PL_CHECK_HIP(hipMemcpy2DAsync(dst, row * 8, h->d.x + h->ndx, (size_t)h->n * 8, (size_t)nu0 * 8, h->B,
                                hipMemcpyDeviceToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpy2DAsync(dst + (size_t)nu0 * 8, row * 8, h->d.xstate, (size_t)h->nx * 8, (size_t)h->nx * 8,
                                h->B, hipMemcpyDeviceToDevice, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_mpc_download(pl_ocp* o, double* host_dst) {
  REQUIRE_DEVICE(o);
  if (!host_dst) { pl_set_error("null argument"); return -1; }
  PlOcpHandle* h = &o->h;
  const int nu0 = o->nodes[0].nu;
  const size_t row = (size_t)nu0 + h->nx, bytes = row * h->B * 8;
  if (stage_reserve(o, bytes, "pl_mpc_download")) return -2;
  char* dst = (char*)o->dl_host;
  PL_CHECK_HIP(hipMemcpy2DAsync(dst, row * 8, h->d.x + h->ndx, (size_t)h->n * 8, (size_t)nu0 * 8, h->B,
                                hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipMemcpy2DAsync(dst + (size_t)nu0 * 8, row * 8, h->d.xstate, (size_t)h->nx * 8, (size_t)h->nx * 8,
                                h->B, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  memcpy(host_dst, o->dl_host, bytes);
  return 0;
}

// ---------------------------------------------------------------------------
// Rollout on the device (record.h, k_record.hip): the log of every step, the per-problem
// metrics and the push schedule.  Their state sits behind the MPC graph key (state.h), and their
// launches run outside the captured step.
static_assert(sizeof(pl_mpc_metrics_t) == sizeof(PlMpcMetrics), "pl_mpc_metrics_t and PlMpcMetrics are one layout");
static const double kNeverOut = 1.7976931348623157e308;  // |z - z_ref| > DBL_MAX, c_z < -DBL_MAX: never

static int tol_check(const char* who, const char* name, const double* v, int count) {
  for (int b = 0; v && b < count; ++b)
    if (!std::isfinite(v[b])) {
      pl_set_error("%s: problem %d: %s = %g is not finite", who, b, name, v[b]);
      return -1;
    }
  return 0;
}

extern "C" int pl_mpc_log_start(pl_ocp* o, long long capacity, int every, const double* dz_tol, const double* cz_min) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (capacity < 0) { pl_set_error("pl_mpc_log_start: capacity %lld is negative", capacity); return -1; }
  if (every < 1) { pl_set_error("pl_mpc_log_start: every = %d, must be at least 1", every); return -1; }
  if (tol_check("pl_mpc_log_start", "dz_tol", dz_tol, o->h.B) || tol_check("pl_mpc_log_start", "cz_min", cz_min, o->h.B))
    return -1;
  PlOcpHandle* h = &o->h;
  const size_t B = h->B;
  const pl::RecLayout L = pl::rec_layout(h->nx, o->nodes[0].nu, h->oc.nfeet);
  const size_t per_slot = B * (size_t)L.row;
  if ((unsigned long long)capacity > (~(size_t)0 / sizeof(double)) / per_slot) {
    pl_set_error("pl_mpc_log_start: capacity %lld x %zu doubles per slot does not fit an allocation", capacity, per_slot);
    return -2;
  }
  REQUIRE_DEVICE(o);
  h->rec_on = 0;
  if (!h->rec_met && (dalloc(o, &h->rec_met, B) || dalloc(o, &h->rec_ref, 3 * B))) return -2;
  const size_t need = (size_t)capacity * per_slot;
  // the stream: an earlier record launch may still write the old log
  if (grow_device(&h->rec_log, &h->rec_log_doubles, need, h->stream, "pl_mpc_log_start")) return -2;
  std::vector<double> tol(2 * B);
  for (size_t b = 0; b < B; ++b) {
    tol[b] = dz_tol ? dz_tol[b] : kNeverOut;
    tol[B + b] = cz_min ? cz_min[b] : -kNeverOut;
  }
  PL_CHECK_HIP(hipMemcpyAsync(h->rec_ref + B, tol.data(), 2 * B * 8, hipMemcpyHostToDevice, h->stream));
  launch_mpc_record_start(h);  // metrics' start values, z_ref from x_state on the device
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));  // tol is read until the copy has run
  h->rec_capacity = capacity;
  h->rec_every = every;
  h->rec_cur[0] = h->rec_cur[1] = h->rec_cur[2] = 0;
  h->rec_on = 1;
  return 0;
}

extern "C" int pl_mpc_log_stop(pl_ocp* o) {
  if (!o) { pl_set_error("null handle"); return -1; }
  o->h.rec_on = 0;
  return 0;
}

extern "C" int pl_mpc_log_sizes(const pl_ocp* o, long long* out) {
  if (!o || !out) { pl_set_error("null argument"); return -1; }
  const PlOcpHandle& h = o->h;
  const pl::RecLayout L = pl::rec_layout(h.nx, o->nodes[0].nu, h.oc.nfeet);
  for (int f = 0; f < PL_REC_FIELDS; ++f) {
    out[2 * f] = L.width[f];
    out[2 * f + 1] = L.off[f];
  }
  out[12] = L.row;
  out[13] = h.rec_capacity;
  out[14] = h.rec_every;
  out[15] = h.rec_cur[1];
  out[16] = h.rec_cur[2];
  return 0;
}

extern "C" int pl_mpc_log_read(pl_ocp* o, long long first_slot, long long count, double* host_dst) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (first_slot < 0 || count < 0 || first_slot > h->rec_cur[1] || count > h->rec_cur[1] - first_slot) {
    pl_set_error("pl_mpc_log_read: slots [%lld, %lld + %lld) outside the %lld recorded", first_slot, first_slot, count,
                 h->rec_cur[1]);
    return -1;
  }
  if (count == 0) return 0;
  if (!host_dst) { pl_set_error("null argument"); return -1; }
  const pl::RecLayout L = pl::rec_layout(h->nx, o->nodes[0].nu, h->oc.nfeet);
  const size_t per_slot = (size_t)h->B * L.row, bytes = (size_t)count * per_slot * 8;
  if (stage_reserve(o, bytes, "pl_mpc_log_read")) return -2;
  PL_CHECK_HIP(hipMemcpyAsync(o->dl_host, h->rec_log + (size_t)first_slot * per_slot, bytes, hipMemcpyDeviceToHost,
                              h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  memcpy(host_dst, o->dl_host, bytes);
  return 0;
}

extern "C" int pl_mpc_log_device(pl_ocp* o, void** ptr) {
  REQUIRE_DEVICE(o);
  if (!ptr) { pl_set_error("null argument"); return -1; }
  PL_CHECK_HIP(hipStreamSynchronize(o->h.stream));
  *ptr = o->h.rec_capacity > 0 ? o->h.rec_log : nullptr;
  return 0;
}

extern "C" int pl_mpc_metrics(pl_ocp* o, pl_mpc_metrics_t* out) {
  REQUIRE_DEVICE(o);
  if (!out) { pl_set_error("null argument"); return -1; }
  PlOcpHandle* h = &o->h;
  if (!h->rec_met) { pl_set_error("pl_mpc_metrics: no log was started (pl_mpc_log_start)"); return -1; }
  PL_CHECK_HIP(hipMemcpyAsync(out, h->rec_met, (size_t)h->B * sizeof(PlMpcMetrics), hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pl_mpc_record_host(const pl_ocp* o, int k, const double* x_init, const double* u0, const pl_stats* stats,
                                  const double* x_state, const double* ground_f, const double* anchors, double z_ref,
                                  const double* dz_tol, const double* cz_min, long long* cursor, double* log,
                                  pl_mpc_metrics_t* metrics) {
  if (!o || !x_init || !u0 || !stats || !x_state || !cursor || !metrics) {
    pl_set_error("pl_mpc_record_host: null argument");
    return -1;
  }
  if (cursor[0] < 0 || cursor[1] < 1 || cursor[2] < 0 || cursor[3] < 0 || cursor[3] > cursor[0] || cursor[4] < 0) {
    pl_set_error("pl_mpc_record_host: cursor {capacity %lld, every %lld, seen %lld, recorded %lld, dropped %lld} is not a log's",
                 cursor[0], cursor[1], cursor[2], cursor[3], cursor[4]);
    return -1;
  }
  if (cursor[0] > 0 && !log) { pl_set_error("pl_mpc_record_host: capacity %lld without a log", cursor[0]); return -1; }
  if (tol_check("pl_mpc_record_host", "dz_tol", dz_tol, 1) || tol_check("pl_mpc_record_host", "cz_min", cz_min, 1))
    return -1;
  const PlOcpHandle& h = o->h;
  // pl_stats back into the kernel's PlProbInfo (fetch_stats is the other direction)
  PlProbInfo info;
  memset(&info, 0, sizeof(info));
  info.status = stats->status;
  info.iter = stats->admm_iters;
  info.ls_accepted = stats->ls_accepted;
  info.ls_alpha = stats->ls_alpha;
  info.viol_max = stats->viol_max;
  info.pri_res = stats->pri_res;
  info.dua_res = stats->dua_res;
  info.f = stats->f;
  const double zero[3 * PL_MAXFEET] = {0.0};
  const pl::RecSrc S{x_init, u0, &info, x_state, ground_f ? ground_f : zero, anchors ? anchors : zero};
  PlMpcMetrics m;
  memcpy(&m, metrics, sizeof(m));
  pl::record_host(h.nx, o->nodes[0].nu, h.oc.nfeet, PL_IS_CV(h.oc.dyn) ? 6 : 0, k, S, z_ref,
                  dz_tol ? *dz_tol : kNeverOut, cz_min ? *cz_min : -kNeverOut, cursor[0], cursor[1], cursor + 2, log, &m);
  memcpy(metrics, &m, sizeof(m));
  return 0;
}

extern "C" int pl_mpc_set_push(pl_ocp* o, const int* k_start, const int* k_end, const double* wrench) {
  if (!o) { pl_set_error("null handle"); return -1; }
  const bool off = !k_start && !k_end && !wrench;
  if (!off && (!k_start || !k_end || !wrench)) {
    pl_set_error("pl_mpc_set_push: k_start, k_end and wrench go together (all NULL switches the schedule off)");
    return -1;
  }
  const size_t B = o->h.B;
  for (size_t b = 0; !off && b < B; ++b) {
    if (k_start[b] < 0 || k_end[b] < 0) {
      pl_set_error("pl_mpc_set_push: problem %zu: window [%d, %d) has a negative step", b, k_start[b], k_end[b]);
      return -1;
    }
    if (k_end[b] < k_start[b]) {
      pl_set_error("pl_mpc_set_push: problem %zu: window [%d, %d) ends before it starts", b, k_start[b], k_end[b]);
      return -1;
    }
    for (int j = 0; j < 6; ++j)
      if (!std::isfinite(wrench[6 * b + j])) {
        pl_set_error("pl_mpc_set_push: problem %zu: wrench[%d] = %g is not finite", b, j, wrench[6 * b + j]);
        return -1;
      }
  }
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  h->dist_wrench_on = 0;  // set or cleared, the schedule overwrites what pl_mpc_set_disturbance left in d.plant_w
  if (off) {
    h->push_on = 0;
    PL_CHECK_HIP(hipMemsetAsync(h->d.plant_w, 0, B * 6 * 8, h->stream));
    PL_CHECK_HIP(hipStreamSynchronize(h->stream));
    return 0;
  }
  if (!h->push_k && (dalloc(o, &h->push_k, 2 * B) || dalloc(o, &h->push_w, 6 * B))) return -2;
  PL_CHECK_HIP(hipMemcpyAsync(h->push_k, k_start, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->push_k + B, k_end, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->push_w, wrench, B * 6 * 8, hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  h->push_on = 1;
  return 0;
}

// ---------------------------------------------------------------------------
// Per-step random state noise and base wrench (noise.h): seeds and sigmas per problem in device
// buffers that k_mpc_prepare alone reads.  Their state sits behind the MPC graph key (state.h),
// like the push schedule's; the draws land in d.plant_noise / d.plant_w, which the handle owns.
static int sigma_check(const char* who, size_t b, const char* name, const double* s, int width) {
  for (int j = 0; s && j < width; ++j)
    if (!std::isfinite(s[j]) || s[j] < 0.0) {
      pl_set_error("%s: problem %zu: %s[%d] = %g is negative or not finite", who, b, name, j, s[j]);
      return -1;
    }
  return 0;
}

extern "C" int pl_mpc_set_noise(pl_ocp* o, const unsigned long long* seed, const double* state_sigma,
                                const double* wrench_sigma) {
  if (!o) { pl_set_error("null handle"); return -1; }
  PlOcpHandle* h = &o->h;
  const size_t B = h->B, ndx = h->ndx;
  if (seed) {
    if (!state_sigma && !wrench_sigma) {
      pl_set_error("pl_mpc_set_noise: seeds without state_sigma and without wrench_sigma (seed == NULL switches the noise off)");
      return -1;
    }
    for (size_t b = 0; b < B; ++b)
      if (sigma_check("pl_mpc_set_noise", b, "state_sigma", state_sigma ? state_sigma + b * ndx : nullptr, (int)ndx) ||
          sigma_check("pl_mpc_set_noise", b, "wrench_sigma", wrench_sigma ? wrench_sigma + b * 6 : nullptr, 6))
        return -1;
    if (state_sigma && h->plant_noise_on) {  // one owner of d.plant_noise
      pl_set_error("pl_mpc_set_noise: a state_noise of pl_mpc_set_disturbance is set and owns the state noise; clear it first");
      return -1;
    }
    if (wrench_sigma && h->dist_wrench_on) {  // one owner of d.plant_w beside the push schedule
      pl_set_error("pl_mpc_set_noise: a base_wrench of pl_mpc_set_disturbance is set and owns the base wrench; clear it first");
      return -1;
    }
  }
  REQUIRE_DEVICE(o);
  const bool wrench_on = seed && wrench_sigma;
  if (seed) {
    if (!h->rng_seed && (dalloc(o, &h->rng_seed, B) || dalloc(o, &h->rng_sigma, B * ndx) || dalloc(o, &h->rng_wsigma, 6 * B)))
      return -2;
    // the stream orders the copies after an earlier prepare launch that still reads the old values
    PL_CHECK_HIP(hipMemcpyAsync(h->rng_seed, seed, B * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    if (state_sigma) PL_CHECK_HIP(hipMemcpyAsync(h->rng_sigma, state_sigma, B * ndx * 8, hipMemcpyHostToDevice, h->stream));
    if (wrench_sigma) PL_CHECK_HIP(hipMemcpyAsync(h->rng_wsigma, wrench_sigma, B * 6 * 8, hipMemcpyHostToDevice, h->stream));
  }
  // the random wrench gone (or everything off) and no schedule that rewrites it: zero = none
  if (!wrench_on && !h->push_on && (!seed || h->rng_wrench_on)) {
    PL_CHECK_HIP(hipMemsetAsync(h->d.plant_w, 0, B * 6 * 8, h->stream));
    h->dist_wrench_on = 0;
  }
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));  // the caller's arrays are read until the copies have run
  h->rng_state_on = seed && state_sigma ? 1 : 0;
  h->rng_wrench_on = wrench_on ? 1 : 0;
  return 0;
}

extern "C" int pl_mpc_get_noise(const pl_ocp* o, int* state_on, int* wrench_on) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (state_on) *state_on = o->h.rng_state_on;
  if (wrench_on) *wrench_on = o->h.rng_wrench_on;
  return 0;
}

extern "C" int pl_mpc_noise_state(pl_ocp* o, double* state_noise, double* base_wrench) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  const size_t nb = (size_t)h->B * h->ndx * 8, wb = (size_t)h->B * 6 * 8;
  if (stage_reserve(o, nb + wb, "pl_mpc_noise_state")) return -2;
  char* st = (char*)o->dl_host;
  PL_CHECK_HIP(hipMemcpyAsync(st, h->d.plant_noise, nb, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(st + nb, h->d.plant_w, wb, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  if (state_noise) memcpy(state_noise, st, nb);
  if (base_wrench) memcpy(base_wrench, st + nb, wb);
  return 0;
}

extern "C" int pl_mpc_noise_host(const pl_ocp* o, int k, unsigned long long seed, const double* state_sigma,
                                 const double* wrench_sigma, const double* det_wrench, const double* x_state,
                                 double* state_noise, double* base_wrench, double* x_init) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (k < 0) { pl_set_error("pl_mpc_noise_host: step %d is negative", k); return -1; }
  if (x_init && !x_state) { pl_set_error("pl_mpc_noise_host: x_init needs x_state"); return -1; }
  const PlOcpHandle& h = o->h;
  if (sigma_check("pl_mpc_noise_host", 0, "state_sigma", state_sigma, h.ndx) ||
      sigma_check("pl_mpc_noise_host", 0, "wrench_sigma", wrench_sigma, 6))
    return -1;
  for (int c = 0; det_wrench && c < 6; ++c)
    if (!std::isfinite(det_wrench[c])) {
      pl_set_error("pl_mpc_noise_host: det_wrench[%d] = %g is not finite", c, det_wrench[c]);
      return -1;
    }
  pl::noise_prepare_host(h.model, h.oc, h.nx, k, seed, state_sigma, wrench_sigma, det_wrench, x_state, state_noise,
                         base_wrench, x_init);
  return 0;
}

extern "C" int pl_rng_block_host(const unsigned* ctr, const unsigned* key, unsigned* out) {
  if (!ctr || !key || !out) { pl_set_error("pl_rng_block_host: null argument"); return -1; }
  pl::philox4x32_10(ctr, key, out);
  return 0;
}

extern "C" int pl_rng_uniforms_host(const unsigned* words, double* u1, double* theta) {
  if (!words || !u1 || !theta) { pl_set_error("pl_rng_uniforms_host: null argument"); return -1; }
  pl::rng_uniforms(words, u1, theta);
  return 0;
}

// ---------------------------------------------------------------------------
// Gait and command timelines (timeline.h): keyframes per problem in device buffers that
// k_mpc_prepare alone reads.  Their state sits behind the MPC graph key (state.h), like the push
// schedule's, and that launch runs outside the captured step.
static_assert(sizeof(pl_mpc_keyframe) == sizeof(PlKeyframe) && sizeof(PlKeyframe) == 128,
              "pl_mpc_keyframe and PlKeyframe are one layout");
static_assert(PL_MPC_MAX_KEYFRAMES == PL_TL_MAXKEY, "one keyframe limit");

// one problem's keyframes [0, count): every refusal of pl_mpc_set_timeline below the counts
static int timeline_check(const char* who, size_t b, const pl_mpc_keyframe* keys, int count) {
  for (int j = 0; j < count; ++j) {
    const pl_mpc_keyframe& K = keys[j];
    if (K.k_start < 0) {
      pl_set_error("%s: problem %zu, keyframe %d: k_start %d is negative", who, b, j, K.k_start);
      return -1;
    }
    if (j > 0 && K.k_start <= keys[j - 1].k_start) {
      pl_set_error("%s: problem %zu, keyframe %d: k_start %d does not increase (keyframe %d starts at %d)", who, b, j,
                   K.k_start, j - 1, keys[j - 1].k_start);
      return -1;
    }
    if (K.gait_type < 0 || K.gait_type > 2) {
      pl_set_error("%s: problem %zu, keyframe %d: gait_type %d outside 0..2", who, b, j, K.gait_type);
      return -1;
    }
    if (!(std::isfinite(K.gait_period) && K.gait_period > 0.0)) {
      pl_set_error("%s: problem %zu, keyframe %d: gait_period %g is not finite and positive", who, b, j, K.gait_period);
      return -1;
    }
    if (!std::isfinite(K.t_shift)) {
      pl_set_error("%s: problem %zu, keyframe %d: t_shift %g is not finite", who, b, j, K.t_shift);
      return -1;
    }
    if (K.ramp != 0 && K.ramp != 1) {
      pl_set_error("%s: problem %zu, keyframe %d: ramp %d is neither 0 nor 1", who, b, j, K.ramp);
      return -1;
    }
    const double* c = K.base_vel_des;  // the 12 commands are contiguous (the layout assert above)
    for (int e = 0; e < PL_TL_NCMD; ++e)
      if (!std::isfinite(c[e])) {
        pl_set_error("%s: problem %zu, keyframe %d: command %d (%s[%d]) = %g is not finite", who, b, j, e,
                     e < 6 ? "base_vel_des" : e < 9 ? "ext_force_des" : "arm_vel_des", e < 6 ? e : e < 9 ? e - 6 : e - 9,
                     c[e]);
        return -1;
      }
  }
  return 0;
}

extern "C" int pl_mpc_set_timeline(pl_ocp* o, int n_key, const pl_mpc_keyframe* keys, const int* count) {
  if (!o) { pl_set_error("null handle"); return -1; }
  const size_t B = o->h.B;
  if (keys) {
    if (n_key < 1 || n_key > PL_TL_MAXKEY) {
      pl_set_error("pl_mpc_set_timeline: n_key %d outside [1, %d]", n_key, PL_TL_MAXKEY);
      return -1;
    }
    for (size_t b = 0; b < B; ++b) {
      const int cnt = count ? count[b] : n_key;
      if (cnt < 1 || cnt > n_key) {
        pl_set_error("pl_mpc_set_timeline: problem %zu: count %d outside [1, %d]", b, cnt, n_key);
        return -1;
      }
      if (timeline_check("pl_mpc_set_timeline", b, keys + b * n_key, cnt)) return -1;
    }
  }
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!keys) {
    h->tl_on = 0;
    return 0;
  }
  if (h->tl_nkey != n_key) {  // another stride: the keyframe buffer is reallocated
    h->tl_on = 0;
    h->tl_nkey = 0;
    size_t have = 0;  // always a new block; the stream: an earlier prepare launch may still read the old one
    if (grow_device(&h->tl_keys, &have, B * n_key, h->stream, "pl_mpc_set_timeline")) return -2;
    h->tl_nkey = n_key;
  }
  if (!h->tl_state) {  // the second of the two: a count buffer left by a failed call is replaced
    size_t nc = 0, ns = 0;
    if (grow_device(&h->tl_count, &nc, B, nullptr, "pl_mpc_set_timeline") ||
        grow_device(&h->tl_state, &ns, B, nullptr, "pl_mpc_set_timeline"))
      return -2;
    PL_CHECK_HIP(hipMemsetAsync(h->tl_state, 0, B * sizeof(PlTimelineState), h->stream));
  }
  // the keyframes each problem owns, the padding zeroed: nothing the caller left there travels
  std::vector<PlKeyframe> hk(B * n_key);
  std::vector<int> hc(B);
  memset(hk.data(), 0, hk.size() * sizeof(PlKeyframe));
  for (size_t b = 0; b < B; ++b) {
    hc[b] = count ? count[b] : n_key;
    memcpy(hk.data() + b * n_key, keys + b * n_key, (size_t)hc[b] * sizeof(PlKeyframe));
  }
  PL_CHECK_HIP(hipMemcpyAsync(h->tl_keys, hk.data(), hk.size() * sizeof(PlKeyframe), hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipMemcpyAsync(h->tl_count, hc.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));  // hk, hc are read until the copies have run
  h->tl_on = 1;
  return 0;
}

extern "C" int pl_mpc_get_timeline(const pl_ocp* o, int* on, int* n_key) {
  if (!o) { pl_set_error("null handle"); return -1; }
  if (on) *on = o->h.tl_on;
  if (n_key) *n_key = o->h.tl_on ? o->h.tl_nkey : 0;
  return 0;
}

extern "C" int pl_mpc_timeline_state(pl_ocp* o, int* seg, int* gait_type, double* gait_period, double* commands) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  if (!h->tl_on) { pl_set_error("pl_mpc_timeline_state: no timeline is set (pl_mpc_set_timeline)"); return -1; }
  const size_t B = h->B, bytes = B * sizeof(PlTimelineState);
  if (stage_reserve(o, bytes, "pl_mpc_timeline_state")) return -2;
  PL_CHECK_HIP(hipMemcpyAsync(o->dl_host, h->tl_state, bytes, hipMemcpyDeviceToHost, h->stream));
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  const PlTimelineState* st = (const PlTimelineState*)o->dl_host;
  for (size_t b = 0; b < B; ++b) {
    if (seg) seg[b] = st[b].seg;
    if (gait_type) gait_type[b] = st[b].gait_type;
    if (gait_period) gait_period[b] = st[b].gait_period;
    if (commands) memcpy(commands + b * PL_TL_NCMD, st[b].cmd, sizeof(st[b].cmd));
  }
  return 0;
}

extern "C" int pl_mpc_timeline_host(const pl_ocp* o, int k, double t0, const pl_mpc_keyframe* keys, int count, double* p,
                                    double* x, int* seg) {
  if (!o || !keys || !p) { pl_set_error("pl_mpc_timeline_host: null argument"); return -1; }
  if (count < 1 || count > PL_TL_MAXKEY) {
    pl_set_error("pl_mpc_timeline_host: count %d outside [1, %d]", count, PL_TL_MAXKEY);
    return -1;
  }
  if (!std::isfinite(t0)) { pl_set_error("pl_mpc_timeline_host: t0 = %g is not finite", t0); return -1; }
  if (timeline_check("pl_mpc_timeline_host", 0, keys, count)) return -1;
  const PlOcpHandle& h = o->h;
  std::vector<PlKeyframe> hk(count);  // exactly the problem's keyframes
  memcpy(hk.data(), keys, (size_t)count * sizeof(PlKeyframe));
  PlTimelineState st;
  pl::timeline_prepare_host(h.model, h.oc, o->nodes.data(), k, t0, hk.data(), count, p, x, &st);
  if (seg) *seg = st.seg;
  return 0;
}

extern "C" int pl_debug_mpc_prepare(pl_ocp* o, int k) {
  REQUIRE_DEVICE(o);
  PlOcpHandle* h = &o->h;
  launch_mpc_prepare(h, k);
  PL_CHECK_HIP(hipGetLastError());
  PL_CHECK_HIP(hipStreamSynchronize(h->stream));
  return 0;
}
