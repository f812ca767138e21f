// Gait and command timelines of the device MPC loop (host+device, fp64): what the gait /
// warm-start launch (k_mpc_prepare) writes into one problem's parameters before MPC step k when
// pl_mpc_set_timeline holds a timeline, and the host restatement pl_mpc_timeline_host runs.
//
// A problem's timeline is `count` keyframes (PlKeyframe = pl_mpc_keyframe, include/pinoloco.h)
// sorted by k_start.  At step k:
//   governing keyframe s   the last one with k_start <= k; before the first keyframe the first
//                          one governs (clamped), so the rule is total (tl_segment).  Entries
//                          past `count` are never read.
//   commands (tl_command)  component j of [base_vel_des 6 | ext_force_des 3 | arm_vel_des 3]:
//                          keyframe s's value, bit for bit, when ramp == 0, when s is the last
//                          keyframe or when k < k_start_s (clamped); otherwise
//                          a = (double)(k - k_s) / (double)(k_{s+1} - k_s), c = c_s + a (c_{s+1} - c_s).
//                          ext_force_des / arm_vel_des are written only where the OCP has the
//                          frame (tl_has_command).
//   gait scalars           n_contacts and swing_period of keyframe s's gait (tl_n_contacts,
//                          tl_swing_period; GaitSequence.__init__, utils/gait_sequence.py:11-21).
//   schedule               pl::gait_schedule over the whole horizon with keyframe s's type and
//                          period at the clock mpc_clock(t0, k, dt_min) + t_shift_s: one gait per
//                          solve, as one n_contacts and one swing_period per solve imply.
//   warm start             forces <- f_des masked by the new schedule (warm_force), k > 0.
// One definition for k_mpc_prepare (k_eval.hip) and the host (timeline_prepare_host).
#pragma once
#include "state.h"
#include "targets.h"

#define PL_TL_MAXKEY 64
#define PL_TL_NCMD 12

// pl_mpc_keyframe (include/pinoloco.h)
struct PlKeyframe {
  int k_start, gait_type, ramp, pad;
  double gait_period, t_shift;
  double cmd[PL_TL_NCMD];  // base_vel_des[6], ext_force_des[3], arm_vel_des[3]
};

// what the last prepare launch used for one problem (pl_mpc_timeline_state)
struct PlTimelineState {
  int seg, gait_type;
  double gait_period;
  double cmd[PL_TL_NCMD];
};

namespace pl {

// The gait clock of MPC step k, t0 + k dt_min rounded once.  The device build has always
// contracted this product and sum into one fused multiply-add; stating the fusion gives the
// host build the same bits.
PL_HD double mpc_clock(double t0, int k, double dt_min) { return __builtin_fma((double)k, dt_min, t0); }

PL_HD int tl_segment(const PlKeyframe* keys, int count, int k) {
  int s = 0;
  while (s + 1 < count && keys[s + 1].k_start <= k) ++s;
  return s;
}

PL_HD double tl_command(const PlKeyframe* keys, int count, int s, int k, int j) {
  const PlKeyframe& K = keys[s];
  if (!K.ramp || s + 1 >= count || k < K.k_start) return K.cmd[j];
  const PlKeyframe& Kn = keys[s + 1];
  const double a = (double)(k - K.k_start) / (double)(Kn.k_start - K.k_start);
  return K.cmd[j] + a * (Kn.cmd[j] - K.cmd[j]);
}

// parameter offset of command component j
PL_HD int tl_command_off(const PlOcpConst& O, int j) {
  return j < 6 ? O.P.base_vel_des + j : j < 9 ? O.P.ext_force_des + (j - 6) : O.P.arm_vel_des + (j - 9);
}
PL_HD bool tl_has_command(const PlOcpConst& O, int j) { return j < 6 || (j < 9 ? O.ext.valid != 0 : O.arm.valid != 0); }

PL_HD double tl_n_contacts(int gait_type) { return gait_type == 0 ? 2.0 : gait_type == 1 ? 3.0 : 4.0; }
PL_HD double tl_swing_period(int gait_type, double period) {
  return gait_type == 0 ? 0.5 * period : gait_type == 1 ? 0.25 * period : period;
}

// Warm start of force component c at node i: f_des, zero on a foot the schedule has in swing
// (ocp_whole_body_rnea.py:207-235).
PL_HD double warm_force(const PlModel& M, const PlOcpConst& O, const double* p, int i, int c) {
  const int foot = c / 3;
  double fd = f_des_comp(M, O, p, c);
  if (foot < 4 && p[O.P.contact + 4 * i + foot] == 0.0) fd = 0.0;
  return fd;
}

// One problem's prepare step on the host (pl_mpc_timeline_host): commands, gait scalars and
// schedule into p, then for k > 0 and x given the masked force warm start into x.
inline void timeline_prepare_host(const PlModel& M, const PlOcpConst& O, const PlNode* nodes, int k, double t0,
                                  const PlKeyframe* keys, int count, double* p, double* x, PlTimelineState* st) {
  const int s = tl_segment(keys, count, k);
  const PlKeyframe& K = keys[s];
  st->seg = s;
  st->gait_type = K.gait_type;
  st->gait_period = K.gait_period;
  for (int j = 0; j < PL_TL_NCMD; ++j) {
    st->cmd[j] = tl_command(keys, count, s, k, j);
    if (tl_has_command(O, j)) p[tl_command_off(O, j)] = st->cmd[j];
  }
  const double sp = tl_swing_period(K.gait_type, K.gait_period);
  p[O.P.n_contacts] = tl_n_contacts(K.gait_type);
  p[O.P.swing_period] = sp;
  const double t = mpc_clock(t0, k, p[O.P.dt_min]) + K.t_shift;
  gait_schedule(O, K.gait_type, K.gait_period, sp, t, p, p + O.P.contact, p + O.P.swing);
  if (k == 0 || !x) return;
  const int fo = u_force_off(O);
  for (int i = 0; i < O.N; ++i)
    for (int c = 0; c < O.nf; ++c) x[nodes[i].x_off + O.ndx + fo + c] = warm_force(M, O, p, i, c);
}

}  // namespace pl
