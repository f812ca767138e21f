// Rollout log of the device MPC loop (host+device, fp64): what one problem's record step
// writes after MPC step k, and the outcome metrics it keeps across steps.
//
// Row (doubles, in this order; rec_layout):
//   x_init[nx]            the believed state the step planned from, p[x_init] (with the state noise)
//   u0[nu_0]              the iterate's node-0 inputs, the doubles pl_mpc_download exports
//   stats[8]              status, admm_iters, ls_accepted, ls_alpha, viol_max, f, pri_res, dua_res
//                         (pl_mpc_get_stats of this step; the interior point's meaning with that solver)
//   x_state[nx]           the true state after the plant: the state of step k + 1
//   ground_f[n_feet 3]    the ground forces of the last substep (zero without contact)
//   anchor_active[n_feet] 1 where the foot's tangential anchor is set
// Every element of a row is one read (rec_elem), so k_mpc_record spreads a row over the lanes
// of a workgroup and stores it coalesced; nothing is recomputed (no retract, no tree pass).
//
// Metrics (rec_metrics, one PlMpcMetrics per problem, updated at every step, logged or not):
//   steps += 1
//   finite = every entry of x_state is finite
//   !finite: first_nonfinite = k if it is still -1; the state joins neither the extrema nor "out"
//   finite:  dz = |z - z_ref|, cz = 1 - 2 (qx^2 + qy^2)   (z the base height, qx, qy of the base
//            quaternion in Pinocchio's order (x, y, z, w); the configuration starts at x[6] for
//            centroidal_vel, x = [h, q], else at x[0])
//            max_dz = max(max_dz, dz), min_cz = min(min_cz, cz)
//            first_out = k if it is still -1 and (dz > dz_tol or cz < cz_min)
//   status != 1: n_not_solved += 1;  ls_accepted == 0: n_ls_rejected += 1
//   viol_max finite: max_viol = max(max_viol, viol_max)
// Start values (rec_metrics_reset): 0 steps, -1, -1, max_dz 0, min_cz 1 (cz <= 1 always), 0, 0, 0.
//
// Slots (rec_slot): the s-th step since the log started is recorded when s % every == 0, into
// the next free slot; with every slot taken it is counted as dropped instead.
// One definition for k_mpc_record (k_record.hip) and the host (pl_mpc_record_host).
#pragma once
#include "ad.h"
#include "state.h"

#define PL_REC_FIELDS 6
#define PL_REC_STATS 8

// pl_mpc_metrics_t (include/pinoloco.h), one per problem
struct PlMpcMetrics {
  int steps, first_nonfinite, first_out, n_not_solved, n_ls_rejected, pad;
  double max_dz, min_cz, max_viol;
};

namespace pl {

struct RecLayout {
  int width[PL_REC_FIELDS], off[PL_REC_FIELDS], row;
};

PL_HD RecLayout rec_layout(int nx, int nu0, int nfeet) {
  RecLayout L;
  const int w[PL_REC_FIELDS] = {nx, nu0, PL_REC_STATS, nx, 3 * nfeet, nfeet};
  int o = 0;
  for (int k = 0; k < PL_REC_FIELDS; ++k) {
    L.width[k] = w[k];
    L.off[k] = o;
    o += w[k];
  }
  L.row = o;
  return L;
}

// what one record step reads; anchors [n_feet][3] (x, y, active), ground_f [n_feet][3]
struct RecSrc {
  const double* x_init;
  const double* u0;
  const PlProbInfo* info;
  const double* x_state;
  const double* ground_f;
  const double* anchors;
};

PL_HD double rec_stat(const PlProbInfo& I, int j) {
  switch (j) {
    case 0: return (double)I.status;
    case 1: return (double)I.iter;
    case 2: return (double)I.ls_accepted;
    case 3: return I.ls_alpha;
    case 4: return I.viol_max;
    case 5: return I.f;
    case 6: return I.pri_res;
    default: return I.dua_res;
  }
}

// element e in [0, L.row) of the row
PL_HD double rec_elem(const RecLayout& L, const RecSrc& S, int e) {
  if (e < L.off[1]) return S.x_init[e];
  if (e < L.off[2]) return S.u0[e - L.off[1]];
  if (e < L.off[3]) return rec_stat(*S.info, e - L.off[2]);
  if (e < L.off[4]) return S.x_state[e - L.off[3]];
  if (e < L.off[5]) return S.ground_f[e - L.off[4]];
  return S.anchors[3 * (e - L.off[5]) + 2] != 0.0 ? 1.0 : 0.0;
}

PL_HD void rec_metrics_reset(PlMpcMetrics& m) {
  m.steps = 0;
  m.first_nonfinite = m.first_out = -1;
  m.n_not_solved = m.n_ls_rejected = m.pad = 0;
  m.max_dz = 0.0;
  m.min_cz = 1.0;
  m.max_viol = 0.0;
}

// finite without <cmath>'s overloads on the device: x - x is 0 for finite x, NaN otherwise
PL_HD bool rec_finite(double x) { return x - x == 0.0; }

// qoff: where the configuration starts in x_state (6 for centroidal_vel, else 0)
PL_HD void rec_metrics(PlMpcMetrics& m, int k, const double* x_state, int nx, int qoff, double z_ref, double dz_tol,
                       double cz_min, const PlProbInfo& I) {
  m.steps += 1;
  bool finite = true;
  for (int j = 0; j < nx; ++j) finite = finite && rec_finite(x_state[j]);
  if (!finite) {
    if (m.first_nonfinite < 0) m.first_nonfinite = k;
  } else {
    const double z = x_state[qoff + 2], qx = x_state[qoff + 3], qy = x_state[qoff + 4];
    double dz = z - z_ref;
    if (dz < 0.0) dz = -dz;
    const double cz = 1.0 - 2.0 * (qx * qx + qy * qy);
    if (dz > m.max_dz) m.max_dz = dz;
    if (cz < m.min_cz) m.min_cz = cz;
    if (m.first_out < 0 && (dz > dz_tol || cz < cz_min)) m.first_out = k;
  }
  if (I.status != 1) m.n_not_solved += 1;
  if (I.ls_accepted == 0) m.n_ls_rejected += 1;
  if (rec_finite(I.viol_max) && I.viol_max > m.max_viol) m.max_viol = I.viol_max;
}

// cur: {seen, recorded, dropped}, advanced by one step; returns the slot to write or -1
PL_HD long long rec_slot(long long capacity, long long every, long long* cur) {
  long long slot = -1;
  if (cur[0] % every == 0) {
    if (cur[1] < capacity) slot = cur[1]++;
    else cur[2] += 1;
  }
  cur[0] += 1;
  return slot;
}

// One problem's record step on the host (pl_mpc_record_host): the row into log[slot][row] of
// this problem's own log when the step gets a slot, and the metrics.  cur as rec_slot.
inline void record_host(int nx, int nu0, int nfeet, int qoff, int k, const RecSrc& S, double z_ref, double dz_tol,
                        double cz_min, long long capacity, long long every, long long* cur, double* log,
                        PlMpcMetrics* met) {
  const RecLayout L = rec_layout(nx, nu0, nfeet);
  const long long slot = rec_slot(capacity, every, cur);
  if (slot >= 0 && log)
    for (int e = 0; e < L.row; ++e) log[(size_t)slot * L.row + e] = rec_elem(L, S, e);
  rec_metrics(*met, k, S.x_state, nx, qoff, z_ref, dz_tol, cz_min, *S.info);
}

}  // namespace pl
