// Retract of one horizon node of a solved OCP (host+device, fp64): the stacked decision
// vector's increments and inputs turned into q, v, a, contact forces, joint torques and the
// base rows of the equations of motion.
//
// retract_stacked_sol / compile_solution of each OCP (ocp_whole_body_rnea.py:293-366,
// ocp_whole_body_acc.py:195-288, ocp_whole_body_aba.py:177-264, ocp_centroidal_vel.py:195-324)
// with the library's own point functions (dyn.h):
//   q, v      x = integrate(x_init, dx_i); centroidal_vel: x = [h, q], v from the inputs or
//             [base_vel_dynamics(h, q, v_j), v_j] without the base (ocp_centroidal_vel.py:228-235)
//   a         the inputs (rnea / acc), [base_acc_dynamics(q, v, a_j, f), a_j] without the base
//             (ocp_whole_body_acc.py:124-135), ABA (aba), a forward difference of the input
//             velocities with the base part from the centroidal base_acc_dynamics
//             (centroidal_vel, ocp_centroidal_vel.py:240-258)
//   tau       u's tau block (rnea, nodes below tau_nodes), u's tau_j (aba), otherwise the joint
//             rows of RNEA(q, v, a, f)
//   eom_base  the base rows of RNEA(q, v, a, f), the tau_b of run_mpc.py:211-233
// Past the reference's compile_solution (which stops at num_steps = 3):
//   centroidal_vel, node N - 1: U[N] does not exist; the difference of the previous node,
//     k = N - 2, with both velocities at this node's h, q (pinoloco/ocp.py OCPCentroidalVel);
//   whole_body_rnea, nodes i >= tau_nodes: no tau variable; tau = RNEA joint rows (run_mpc.py:211, 233);
//   whole_body_rnea with include_acc = False: a = (v_{i+1} - v_i) / dt_i inside RNEA
//     (ocp_whole_body_rnea.py:183-191), not an output (u_sol[:0]).
// One definition for the CasADi export's retract_solution (api_casadi.hip, host, problem 0) and
// k_retract (k_retract.hip, one thread per problem and node).
#pragma once
#include "dyn.h"
#include "state.h"

namespace pl {

// Destination rows of one node: element k of a field at ptr[k * stride]; a null field is not
// wanted (and what only it needs is not computed).
struct RetractOut {
  double *q, *v, *a, *f, *tau, *eom;
  int stride;
};

// Packed result of a whole batch, field-major: q | v | a | forces | tau | eom_base, each field
// [batch][rows][width] (doubles).  rows = steps, plus the terminal node's row for q and, where
// v is part of the state, for v (centroidal_vel: v comes from the inputs, steps rows,
// pinoloco/ocp.py OCPCentroidalVel); a has no columns for whole_body_rnea with include_acc = False.
#define PL_RETRACT_FIELDS 6
struct RetractLayout {
  long long width[PL_RETRACT_FIELDS], rows[PL_RETRACT_FIELDS], off[PL_RETRACT_FIELDS], total;
};
inline RetractLayout retract_layout(const PlOcpConst& O, int batch, int steps, int terminal) {
  RetractLayout L;
  const long long w[PL_RETRACT_FIELDS] = {O.nq, O.nv, O.dyn == PL_DYN_RNEAFD ? 0 : O.nv, O.nf, O.nj, 6};
  long long off = 0;
  for (int k = 0; k < PL_RETRACT_FIELDS; ++k) {
    L.width[k] = w[k];
    L.rows[k] = steps + ((k == 0 || (k == 1 && !PL_IS_CV(O.dyn))) && terminal ? 1 : 0);
    L.off[k] = off;
    off += (long long)batch * L.rows[k] * L.width[k];
  }
  L.total = off;
  return L;
}

// Node i of the problem with parameters p and decision vector x.  i == N is the terminal
// node: q, and v where it is part of the state.  dyn = O.dyn (a constant in the kernels).
PL_HD void retract_node(const PlModel& M, const PlOcpConst& O, int dyn, const PlNode* nodes, int N, const double* p,
                        const double* x, const double* x_init, int i, const RetractOut& out) {
  const int nq = M.nq, nv = M.nv, nj = O.nj, s = out.stride;
  const bool cv = PL_IS_CV(dyn);
  double xs[PL_MAXQ + PL_MAXV], a[PL_MAXV], tau[PL_MAXV], vfull[PL_MAXV], vnext[PL_MAXV];
  PlFrameRef F0;
  F0.joint = 0;
  F0.valid = 0;
  for (int k = 0; k < 9; ++k) F0.R[k] = 0.0;
  for (int k = 0; k < 3; ++k) F0.p[k] = 0.0;
  const double* dx = x + nodes[i].x_off;
  dyn_eval(M, O, F0, cv ? PL_FN_INTEGRATE_CV : PL_FN_INTEGRATE_WB, 0, x_init, dx, nullptr, nullptr, xs);
  const double* q = cv ? xs + 6 : xs;
  if (out.q) for (int k = 0; k < nq; ++k) out.q[k * s] = q[k];
  if (i >= N) {
    if (out.v && !cv) for (int k = 0; k < nv; ++k) out.v[k * s] = xs[nq + k];
    return;
  }
  const double* u = dx + O.ndx;
  const int na = PL_IS_RNEA(dyn) ? O.na : (dyn == PL_DYN_ACC || dyn == PL_DYN_CA || dyn == PL_DYN_ACCNB) ? O.na
                 : (dyn == PL_DYN_CV ? nv : (dyn == PL_DYN_CVNB ? nj : 0));
  const double* v = cv ? u : xs + nq;
  const double* f = u + (dyn == PL_DYN_ABA ? nj : na);
  if (dyn == PL_DYN_CVNB) {  // v = [base_vel_dynamics(h, q, v_j), v_j] (ocp_centroidal_vel.py:228-235)
    dyn_eval(M, O, F0, PL_FN_BASE_VEL_CV, 0, xs, q, u, nullptr, vfull);
    for (int k = 0; k < nj; ++k) vfull[6 + k] = u[k];
    v = vfull;
  }
  const bool tau_in_u = (PL_IS_RNEA(dyn) && i < O.tau_nodes) || dyn == PL_DYN_ABA;
  const bool want_rnea = out.eom || (out.tau && !tau_in_u);
  const bool want_a = want_rnea || (out.a && dyn != PL_DYN_RNEAFD);
  if (want_a) {
    switch (dyn) {
      case PL_DYN_ABA:
        dyn_eval(M, O, F0, PL_FN_ABA, 0, q, v, u, f, a);
        break;
      case PL_DYN_CV:
      case PL_DYN_CVNB: {
        // forward difference of the input velocities; the last node reuses the previous
        // node's difference (there is no U[N])
        const int kd = i + 1 < N ? i : i - 1;
        const double dt = node_dt(O, p, kd);
        const double* u0 = x + nodes[kd].x_off + O.ndx;
        const double* un = x + nodes[kd + 1].x_off + O.ndx;
        if (dyn == PL_DYN_CVNB) {  // both v_b from this node's h, q (ocp_centroidal_vel.py:240-246)
          dyn_eval(M, O, F0, PL_FN_BASE_VEL_CV, 0, xs, q, un, nullptr, vnext);
          for (int k = 0; k < nj; ++k) vnext[6 + k] = un[k];
          un = vnext;
          if (kd != i) {
            dyn_eval(M, O, F0, PL_FN_BASE_VEL_CV, 0, xs, q, u0, nullptr, a);
            for (int k = 0; k < nj; ++k) a[6 + k] = u0[k];
            u0 = a;
          } else {
            u0 = v;
          }
        }
        for (int k = 0; k < nv; ++k) a[k] = (un[k] - u0[k]) / dt;
        dyn_eval(M, O, F0, PL_FN_BASE_ACC_CV, 0, q, v, a + 6, f, a);
      } break;
      case PL_DYN_ACCNB:  // a = [base_acc_dynamics(q, v, a_j, f), a_j] (ocp_whole_body_acc.py:124-135)
        for (int k = 0; k < nj; ++k) a[6 + k] = u[k];
        dyn_eval(M, O, F0, PL_FN_BASE_ACC_WB, 0, q, v, u, f, a);
        break;
      case PL_DYN_RNEAFD: {  // a = (v_{i+1} - v_i) / dt_i (ocp_whole_body_rnea.py:183-191)
        const double dt = node_dt(O, p, i);
        const double* dvn = x + nodes[i + 1].x_off + nv;
        for (int k = 0; k < nv; ++k) a[k] = ((x_init[nq + k] + dvn[k]) - v[k]) / dt;
      } break;
      default:
        for (int k = 0; k < nv; ++k) a[k] = u[k];
    }
  }
  if (want_rnea) dyn_eval(M, O, F0, PL_FN_RNEA, 0, q, v, a, f, tau);
  if (out.v) for (int k = 0; k < nv; ++k) out.v[k * s] = v[k];
  if (out.a && dyn != PL_DYN_RNEAFD) for (int k = 0; k < nv; ++k) out.a[k * s] = a[k];
  if (out.f) for (int k = 0; k < O.nf; ++k) out.f[k * s] = f[k];
  if (out.tau) {
    for (int k = 0; k < nj; ++k) {
      double t;
      if (tau_in_u) t = PL_IS_RNEA(dyn) ? u[na + O.nf + k] : u[k];
      else t = tau[6 + k];
      out.tau[k * s] = t;
    }
  }
  if (out.eom) for (int k = 0; k < 6; ++k) out.eom[k * s] = tau[k];
}

}  // namespace pl
