// Plant of the device MPC loop (host+device, fp64): one problem's true state stepped through
// the forward dynamics under the torques and contact forces the solve of this step commands.
//
// The reference closes its loop on the optimiser's own prediction, x_init <- integrate(x_init,
// DX[1]) (run_mpc.py:142, k_mpc_finish); the noise it leaves commented out (run_mpc.py:79-82)
// and the dt_min it documents as "used for simulation" point at a simulated plant.  Here:
//   tau_cmd, f_cmd  node 0 of the retract (retract.h): u's tau block where it exists, else the
//                   joint rows of RNEA at the believed state x_init; the forces of u, world-aligned
//                   at the contact frames (feet, then the external-force frame)
//   (q, v)          the true state x_state, not x_init (they differ under state noise)
//   h               dt_min / substeps, the problem's own dt_min
//   substeps x      a = ABA(q, v, [w_b; tau_cmd], f_cmd); q <- integrate(q, v h); v <- v + a h
// explicit Euler with the old v, the OCP's own discretisation (ocp_whole_body_rnea.py:155-158).
// w_b is the generalised force on v[0:6] of the free-flyer (linear then angular, base frame);
// aba_forward re-expresses f_cmd at each substep's q (dynamics_whole_body_torque.py:55-69).
// Defined on x = [q, v]: every dynamics kind but centroidal_vel (x = [h, q]).
//
// With contact (plant_step<true>, pl_mpc_set_contact) the feet get the ground's force instead of
// the commanded one and the joint torque a PD term towards node 1 of the plan, the q, v, tau
// that compile_solution exports for a joint-level controller (ocp_whole_body_rnea.py:326-366).
// Per substep and foot e, in this order (ground_force below):
//   p = world position of the foot frame, u = its LOCAL_WORLD_ALIGNED linear velocity
//   d = ground_z[e] - p.z
//   !(d > 0): f_e = 0, anchor[e].active = 0                       in the air (lift-off)
//   else  fn = max(0, k_n d - d_n u.z)
//         !anchor[e].active: anchor[e].xy = p.xy, active = 1      touchdown
//         ft = -k_t (p.xy - anchor[e].xy) - d_t u.xy
//         lim = mu fn, nrm = sqrt(ft.x^2 + ft.y^2)
//         nrm > lim: ft *= lim / nrm;                             sliding: clamped to the cone,
//                    k_t > 0: anchor[e].xy = p.xy + (ft + d_t u.xy) / k_t   the anchor dragged
//         f_e = (ft.x, ft.y, fn)
//   tau_j = tau_cmd + kp (q_des - q_j) + kd (v_des - v_j)
// q_des, v_des: the joint parts of node 1 of the same retract (believed state), held over the
// step; the external-force frame keeps its commanded force.  The forces come out of
// aba_forward's first pass (rbd.h AbaForceSource), which has the foot joint's rotation and
// velocity at hand and carries the joint's world position for this use: no second kinematics
// pass.  The anchors ([n_feet][3]: x, y, active) are plant state across substeps and steps.
// The explicit damping term bounds the step: h d_n / m_foot < 2.
// One definition for k_plant (k_plant.hip, one thread per problem) and host callers.
#pragma once
#include "retract.h"

namespace pl {

// the ground's force on one foot; anchor = (x, y, active) of this foot, updated in place
PL_HD void ground_force(const PlContact& c, double gz, const double* p, const double* u, double* anchor, double* f) {
  const double d = gz - p[2];
  if (!(d > 0.0)) {
    f[0] = f[1] = f[2] = 0.0;
    anchor[2] = 0.0;
    return;
  }
  double fn = c.k_n * d - c.d_n * u[2];
  if (!(fn > 0.0)) fn = 0.0;
  if (anchor[2] == 0.0) {
    anchor[0] = p[0];
    anchor[1] = p[1];
    anchor[2] = 1.0;
  }
  double ftx = -c.k_t * (p[0] - anchor[0]) - c.d_t * u[0];
  double fty = -c.k_t * (p[1] - anchor[1]) - c.d_t * u[1];
  const double lim = c.mu * fn, nrm = sqrt(ftx * ftx + fty * fty);
  if (nrm > lim) {
    const double sc = lim / nrm;
    ftx *= sc;
    fty *= sc;
    if (c.k_t > 0.0) {
      anchor[0] = p[0] + (ftx + c.d_t * u[0]) / c.k_t;
      anchor[1] = p[1] + (fty + c.d_t * u[1]) / c.k_t;
    }
  }
  f[0] = ftx;
  f[1] = fty;
  f[2] = fn;
}

// aba_forward's force source under contact: the ground at the feet, the command elsewhere
struct GroundForces {
  const PlContact* c;
  const double* ground_z;  // [n_feet]
  double* anchors;         // [n_feet][3], in/out
  double* f_out;           // [n_feet][3]: the ground forces of this call
  const double* f_cmd;     // [3 nee]: read for the external-force frame only
  int nfeet;
};
template <> struct AbaForceSource<GroundForces> { static constexpr bool kFromMotion = true; };
PL_HD void aba_point_force(const GroundForces& G, int e, const PlFrameRef& F, const double* oRj, const double* opj,
                           const double* vj, double* fw) {
  if (e >= G.nfeet) {
    for (int k = 0; k < 3; ++k) fw[k] = G.f_cmd[3 * e + k];
    return;
  }
  double t[3], p[3], wxp[3], u[3];
  matvec(oRj, F.p, t);
  for (int k = 0; k < 3; ++k) p[k] = opj[k] + t[k];
  cross3(vj + 3, F.p, wxp);
  const double lv[3] = {vj[0] + wxp[0], vj[1] + wxp[1], vj[2] + wxp[2]};
  matvec(oRj, lv, u);
  ground_force(*G.c, G.ground_z[e], p, u, G.anchors + 3 * e, fw);
  for (int k = 0; k < 3; ++k) G.f_out[3 * e + k] = fw[k];
}

// kContact = false: contact, ground_z, anchors and f_ground are not read.
template <bool kContact = false>
PL_HD void plant_step(const PlModel& M, const PlOcpConst& O, int dyn, const PlNode* nodes, int N, const double* p,
                      const double* x, const double* base_wrench, int substeps, double* x_state,
                      const PlContact* contact = nullptr, const double* ground_z = nullptr,
                      double* anchors = nullptr, double* f_ground = nullptr) {
  const int nq = M.nq, nv = M.nv;
  double tau[PL_MAXV], f[3 * (PL_MAXFEET + 1)];
  const RetractOut cmd{nullptr, nullptr, nullptr, f, tau, nullptr, 1};
  retract_node(M, O, dyn, nodes, N, p, x, p + O.P.x_init, 0, cmd);
  double q[PL_MAXQ], qn[PL_MAXQ], v[PL_MAXV], a[PL_MAXV], dq[PL_MAXV];
  for (int k = 0; k < nq; ++k) q[k] = x_state[k];
  for (int k = 0; k < nv; ++k) v[k] = x_state[nq + k];
  const double h = p[O.P.dt_min] / (double)substeps;
  double qd[kContact ? PL_MAXQ : 1], vd[kContact ? PL_MAXV : 1], tpd[kContact ? PL_MAXV : 1];
  if constexpr (kContact) {
    const RetractOut des{qd, vd, nullptr, nullptr, nullptr, nullptr, 1};
    retract_node(M, O, dyn, nodes, N, p, x, p + O.P.x_init, 1, des);
  }
  for (int s = 0; s < substeps; ++s) {
    if constexpr (kContact) {
      for (int k = 0; k < O.nj; ++k)
        tpd[k] = tau[k] + contact->kp * (qd[7 + k] - q[7 + k]) + contact->kd * (vd[6 + k] - v[6 + k]);
      const GroundForces G{contact, ground_z, anchors, f_ground, f, O.nfeet};
      aba_forward<double>(M, O, q, v, ArrIn{tpd}, G, a, ArrIn{base_wrench});
    } else {
      aba_forward<double>(M, O, q, v, ArrIn{tau}, ArrIn{f}, a, ArrIn{base_wrench});
    }
    for (int k = 0; k < nv; ++k) dq[k] = v[k] * h;
    const VecIn<double> step{dq, nullptr, 0.0, -1};
    integrate_q<double>(M, q, step, qn);
    for (int k = 0; k < nq; ++k) q[k] = qn[k];
    for (int k = 0; k < nv; ++k) v[k] += a[k] * h;
  }
  for (int k = 0; k < nq; ++k) x_state[k] = q[k];
  for (int k = 0; k < nv; ++k) x_state[nq + k] = v[k];
}

}  // namespace pl
