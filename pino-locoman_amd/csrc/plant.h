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
// One definition for k_plant (k_plant.hip, one thread per problem) and host callers.
#pragma once
#include "retract.h"

namespace pl {

PL_HD void plant_step(const PlModel& M, const PlOcpConst& O, int dyn, const PlNode* nodes, int N, const double* p,
                      const double* x, const double* base_wrench, int substeps, double* x_state) {
  const int nq = M.nq, nv = M.nv;
  double tau[PL_MAXV], f[3 * (PL_MAXFEET + 1)];
  const RetractOut cmd{nullptr, nullptr, nullptr, f, tau, nullptr, 1};
  retract_node(M, O, dyn, nodes, N, p, x, p + O.P.x_init, 0, cmd);
  double q[PL_MAXQ], qn[PL_MAXQ], v[PL_MAXV], a[PL_MAXV], dq[PL_MAXV];
  for (int k = 0; k < nq; ++k) q[k] = x_state[k];
  for (int k = 0; k < nv; ++k) v[k] = x_state[nq + k];
  const double h = p[O.P.dt_min] / (double)substeps;
  for (int s = 0; s < substeps; ++s) {
    aba_forward<double>(M, O, q, v, ArrIn{tau}, ArrIn{f}, a, ArrIn{base_wrench});
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
