// Jacobians of the Dynamics plugin's point functions (include/pinoloco.h, pl_dyn_jac), host+device.
//
// The reference differentiates its point functions with ca.jacobian when an OCP uses them in a
// row (optimization/ocp.py:283-284).  Here one Jacobian column is one forward-mode pass in dual
// numbers (ad.h) over the scalar-templated tree passes of rbd.h, seeded on one tangent direction
// of one input:
//   * a Euclidean input (v, a, forces, tau_j, h, ...): the unit vector of the column;
//   * the configuration q: the tangent of integrate(q, eps e_c) at eps = 0 (pinocchio's local
//     free-flyer twist, linear then angular; revolute coordinates add), the convention of
//     computeRNEADerivatives and of the OCP's own dq columns.  The free-flyer part comes from
//     integrate_ff<Dual>; every column is evaluated at q itself (the value part of
//     integrate(q, 0) differs from q by round-off only and is not used).
// Families (one kernel instantiation each, k_dyn_jac.hip):
//   TREE   rnea, nle, whole-body gaps: tree_pass<Dual>;
//   COMP   centroidal_acc gaps (the total wrench at the CoM) and both base accelerations (the six
//          base equations solved by base_solve<Dual>): tree_pass<Dual> with the composite sums.
//          The centroidal_vel base acceleration A_b^-1 (dh - dA v - A_j a_j) is the same six
//          equations written about the CoM, so it shares the whole-body column;
//   ABA    the implicit function: with a* = M^-1 ([0; tau_j] - RNEA(q, v, 0, f)) from the primal
//          Cholesky factor of M (built once per point from RNEA columns, as k_eval_jac<ABA>
//          does), column = M^-1 d/ds ([0; tau_j] - RNEA(q, v, a*, f)): one dual tree pass and
//          one solve with the shared factor;
//   CEN    com_dynamics, centroidal_vel gaps, base_vel_dynamics, centre of mass: centroidal_pass<Dual>;
//   FRAME  frame position / velocity: a walk that carries one joint's dual state down its chain.
#pragma once
#include "dyn.h"

namespace pl {

enum { PL_JF_NONE = -1, PL_JF_TREE = 0, PL_JF_COMP, PL_JF_ABA, PL_JF_CEN, PL_JF_FRAME, PL_JF_COUNT };

PL_HD int dyn_jac_family(int fn) {
  switch (fn) {
    case PL_FN_RNEA: case PL_FN_NLE: case PL_FN_GAPS_WB: return PL_JF_TREE;
    case PL_FN_GAPS_CA: case PL_FN_BASE_ACC_WB: case PL_FN_BASE_ACC_CV: return PL_JF_COMP;
    case PL_FN_ABA: return PL_JF_ABA;
    case PL_FN_COM_DYN: case PL_FN_GAPS_CV: case PL_FN_BASE_VEL_CV: case PL_FN_COM: return PL_JF_CEN;
    case PL_FN_FRAME_POS: case PL_FN_FRAME_VEL: return PL_JF_FRAME;
    default: return PL_JF_NONE;  // matrix-valued functions and the state maps
  }
}
// The input that is a configuration (tangent length nv); every other input is Euclidean.
PL_HD int dyn_jac_cfg_input(int fn) { return (fn == PL_FN_BASE_VEL_CV || fn == PL_FN_GAPS_CV) ? 1 : 0; }
PL_HD void dyn_jac_tan_len(const PlModel& M, int fn, int nf, int* in_len, int* tan_len) {
  dyn_in_len(M, fn, nf, in_len);
  for (int k = 0; k < 4; ++k) tan_len[k] = in_len[k];
  tan_len[dyn_jac_cfg_input(fn)] = M.nv;
}
// Column `col` of the Jacobian with respect to the inputs of `wrt`: its input and local column.
PL_HD void dyn_jac_locate(const int* tan_len, unsigned wrt, int col, int* input, int* local) {
  *input = -1;
  *local = 0;
  for (int k = 0; k < 4; ++k) {
    if (!((wrt >> k) & 1u)) continue;
    if (col < tan_len[k]) { *input = k; *local = col; return; }
    col -= tan_len[k];
  }
}

// Dual inputs: a[k - off] (zero below off and for a null array) with the tangent on entry `seed`.
struct SeedIn {
  const double* a;
  int seed, off;
  PL_HD Dual operator[](int k) const {
    if (!a || k < off) return Dual(0.0);
    return Dual(a[k - off], k - off == seed ? 1.0 : 0.0);
  }
};
struct SeedQ {  // revolute coordinates of q, seed = the q index carrying the tangent
  const double* q;
  int seed;
  PL_HD Dual operator()(int k) const { return Dual(q[k], k == seed ? 1.0 : 0.0); }
};
struct UnitTan {  // the tangent eps e_seed at eps = 0
  int seed;
  PL_HD Dual operator[](int k) const { return Dual(0.0, k == seed ? 1.0 : 0.0); }
};
struct UnitD {  // e_k in double (k < 0: zero)
  int k;
  PL_HD double operator[](int j) const { return j == k ? 1.0 : 0.0; }
};

// q with the tangent of integrate(q, eps e_c) (c < 0: no tangent).
PL_HD void seed_config(const double* q, int c, Dual* qb, SeedQ* qr) {
  for (int k = 0; k < 7; ++k) qb[k] = Dual(q[k]);
  if (c >= 0 && c < 6) {
    Dual t[7];
    integrate_ff<Dual>(q, UnitTan{c}, t);
    for (int k = 0; k < 7; ++k) qb[k].d = t[k].d;
  }
  *qr = SeedQ{q, c >= 6 ? c + 1 : -1};
}

// The dual state (world placement, local velocity) of joint J, carried down its chain.
template <class VA>
PL_HD void joint_walk(const PlModel& M, const Dual* qb, const SeedQ& qr, const VA& v, bool want_v, int J, Dual* oR,
                      Dual* op, Dual* vl) {
  quat_to_R(qb + 3, oR);
  for (int k = 0; k < 3; ++k) op[k] = qb[k];
  for (int k = 0; k < 6; ++k) vl[k] = want_v ? v[k] : Dual(0.0);
  for (int ch = 0; ch < M.nchains; ++ch) {
    const int first = M.chain_first[ch];
    if (J < first || J >= first + M.chain_len[ch]) continue;
    for (int j = first; j <= J; ++j) {
      Dual s, c, Rl[9], vj[6], oRj[9], t3[3];
      sincos_s(qr(M.idx_q[j]), &s, &c);
      rev_rot(M, j, s, c, Rl);
      act_inv_motion(Rl, M.jp[j], vl, vj);
      if (want_v) {
        const Dual qd = v[M.idx_v[j]];
        for (int k = 0; k < 3; ++k) vj[3 + k] += M.axis[j][k] * qd;
      }
      matmul3(oR, Rl, oRj);
      matvec(oR, M.jp[j], t3);
      for (int k = 0; k < 3; ++k) op[k] = op[k] + t3[k];
      for (int k = 0; k < 9; ++k) oR[k] = oRj[k];
      for (int k = 0; k < 6; ++k) vl[k] = vj[k];
    }
  }
}

// x <- L^-T L^-1 x for a strided x (chol_solve of rows.h on a lane's slots of a shared store)
PL_HD void chol_solve_strided(const double* L, int n, double* x, int stride) {
  for (int i = 0; i < n; ++i) {
    const double* Li = L + i * (i + 1) / 2;
    double t = x[i * stride];
    for (int k = 0; k < i; ++k) t -= Li[k] * x[k * stride];
    x[i * stride] = t / Li[i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = x[i * stride];
    for (int k = i + 1; k < n; ++k) t -= L[k * (k + 1) / 2 + i] * x[k * stride];
    x[i * stride] = t / L[i * (i + 1) / 2 + i];
  }
}

// Shared primal of a point's ABA columns, split so that a wave spreads the RNEA passes over its
// lanes: column c < nv is M e_c + t0, c = nv is t0 = RNEA(q, 0, 0), c = nv + 1 is
// RNEA(q, v, 0, f) (raw: (nv + 2) x nv); aba_factor_solve (dyn.h) turns raw into PL_ABA_SH.
#define PL_ABA_RAW ((PL_MAXV + 2) * PL_MAXV)
PL_HD void aba_point_column(const PlModel& M, const PlOcpConst& O, const double* q, const double* v, const double* f,
                            int c, NodeKin<double>& kin, double* out) {
  const int nv = M.nv;
  const bool full = c > nv;
  const RevQArr<double> qr{q};
  tree_pass<double>(M, O, q, qr, ArrIn{full ? v : nullptr}, UnitD{c < nv ? c : -1}, ArrIn{full ? f : nullptr}, true,
                    false, kin);
  for (int k = 0; k < 6; ++k) out[k] = kin.tau[k];
  for (int k = 6; k < nv; ++k) out[k] = kin.tau_j(k - 6);
}

// Rows of a function's Jacobian (= its output length).
PL_HD int dyn_jac_rows(const PlModel& M, int fn) { return dyn_out_len(M, fn); }

// One Jacobian column: input `k`, local tangent column `c`; row r goes to out[r * ostride].
// kin: a NodeKin<Dual> store (PL_KIN_STORE entries; TREE / COMP / ABA); aba_sh: the point's shared
// primal (ABA).  FAM is dyn_jac_family(fn).
template <int FAM>
PL_HD void dyn_jac_column(const PlModel& M, const PlOcpConst& O, const PlFrameRef& F, int fn, int flags,
                          const double* in0, const double* in1, const double* in2, const double* in3, int k, int c,
                          NodeKin<Dual>& kin, const double* aba_sh, double* out, size_t ostride) {
  const int nv = M.nv, nj = M.nq - 7;
  const int cfg = dyn_jac_cfg_input(fn);
  const int s0 = k == 0 ? c : -1, s1 = k == 1 ? c : -1, s2 = k == 2 ? c : -1, s3 = k == 3 ? c : -1;
  Dual qb[7];
  SeedQ qr;
  seed_config(cfg == 0 ? in0 : in1, k == cfg ? c : -1, qb, &qr);
  if constexpr (FAM == PL_JF_TREE) {
    const bool nle = fn == PL_FN_NLE;
    tree_pass<Dual>(M, O, qb, qr, SeedIn{in1, s1, 0}, SeedIn{nle ? nullptr : in2, s2, 0},
                    SeedIn{nle ? nullptr : in3, s3, 0}, true, false, kin);
    for (int r = 0; r < 6; ++r) out[r * ostride] = kin.tau[r].d;
    if (fn != PL_FN_GAPS_WB)
      for (int r = 6; r < nv; ++r) {
        const Dual t = kin.tau_j(r - 6);
        out[r * ostride] = t.d;
      }
  } else if constexpr (FAM == PL_JF_COMP) {
    Dual comp[15], res[6];
    const bool gap = fn == PL_FN_GAPS_CA;
    tree_pass<Dual>(M, O, qb, qr, SeedIn{in1, s1, 0}, SeedIn{in2, s2, gap ? 0 : 6}, SeedIn{in3, s3, 0}, true, false,
                    kin, comp, std::true_type{});
    if (gap) {
      centroidal_gap(M.total_mass, qb, comp, res);
    } else {
      Dual R0[9];
      quat_to_R(qb + 3, R0);
      base_solve(M.total_mass, R0, comp, kin.tau, res);
    }
    for (int r = 0; r < 6; ++r) out[r * ostride] = res[r].d;
  } else if constexpr (FAM == PL_JF_ABA) {
    tree_pass<Dual>(M, O, qb, qr, SeedIn{in1, s1, 0}, ShAcc{aba_sh}, SeedIn{in3, s3, 0}, true, false, kin);
    // the right-hand side in the lane's chain slots of the store (free once the pass is done)
    double* x = kin.dst + (PL_MAXV - 6 + 3 * PL_MAXFEET) * kin.dstride;
    for (int r = 0; r < 6; ++r) x[r * kin.dstride] = -kin.tau[r].d;
    for (int r = 0; r < nj; ++r) {
      const Dual t = kin.tau_j(r);
      x[(6 + r) * kin.dstride] = (r == s2 ? 1.0 : 0.0) - t.d;
    }
    chol_solve_strided(aba_sh + PL_MAXV, nv, x, kin.dstride);
    for (int r = 0; r < nv; ++r) out[r * ostride] = x[r * kin.dstride];
  } else if constexpr (FAM == PL_JF_CEN) {
    Dual hg[6], hd[6], ci[9];
    if (fn == PL_FN_COM_DYN) {
      centroidal_pass<Dual>(M, O, qb, qr, SeedIn{nullptr, -1, 0}, SeedIn{in1, s1, 0}, false, true, hg, hd);
      for (int r = 0; r < 6; ++r) out[r * ostride] = hd[r].d;
    } else if (fn == PL_FN_GAPS_CV) {
      centroidal_pass<Dual>(M, O, qb, qr, SeedIn{in2, s2, 0}, SeedIn{nullptr, -1, 0}, true, false, hg, hd);
      for (int r = 0; r < 6; ++r) out[r * ostride] = hg[r].d - (r == s0 ? M.total_mass : 0.0);
    } else if (fn == PL_FN_BASE_VEL_CV) {
      centroidal_pass<Dual>(M, O, qb, qr, SeedIn{in2, s2, 6}, SeedIn{nullptr, -1, 0}, true, false, hg, hd, ci,
                            std::true_type{});
      Dual R0[9], h[6], vb[6];
      quat_to_R(qb + 3, R0);
      for (int r = 0; r < 6; ++r) h[r] = Dual(in0[r], r == s0 ? 1.0 : 0.0);
      base_vel_solve(M.total_mass, R0, qb, ci, h, hg, vb);
      for (int r = 0; r < 6; ++r) out[r * ostride] = vb[r].d;
    } else {  // PL_FN_COM
      centroidal_pass<Dual>(M, O, qb, qr, SeedIn{nullptr, -1, 0}, SeedIn{nullptr, -1, 0}, false, false, hg, hd, ci,
                            std::true_type{});
      for (int r = 0; r < 3; ++r) out[r * ostride] = ci[r].d;
    }
  } else if constexpr (FAM == PL_JF_FRAME) {
    const bool vel = fn == PL_FN_FRAME_VEL, rel = vel && (flags & 2);
    const SeedIn v{vel ? in1 : nullptr, s1, 0};
    Dual oR[9], op[3], vl[6];
    joint_walk(M, qb, qr, v, vel, F.joint, oR, op, vl);
    if (!vel) {
      Dual R[9], p[3];
      frame_placement(oR, op, F, R, p);
      for (int r = 0; r < 3; ++r) out[r * ostride] = p[r].d;
    } else {
      Dual res[6];
      if (rel) {
        Dual bR[9], bp[3], bv[6];
        joint_walk(M, qb, qr, v, true, O.base.joint, bR, bp, bv);
        frame_velocity(oR, op, vl, F, bR, bp, bv, O.base, true, res);
      } else {
        frame_velocity(oR, op, vl, F, oR, op, vl, O.base, false, res);
      }
      for (int r = 0; r < 6; ++r) out[r * ostride] = res[r].d;
    }
  }
}

// Host form: every selected column of one point, jac row-major [rows][W].
inline void dyn_jac_point(const PlModel& M, const PlOcpConst& O, const PlFrameRef& F, int fn, int flags, unsigned wrt,
                         const double* in0, const double* in1, const double* in2, const double* in3, double* jac) {
  int in_len[4], tan_len[4], W = 0;
  dyn_jac_tan_len(M, fn, O.nf, in_len, tan_len);
  for (int k = 0; k < 4; ++k)
    if ((wrt >> k) & 1u) W += tan_len[k];
  const int fam = dyn_jac_family(fn);
  double st[2 * PL_KIN_STORE];  // interleaved (value, tangent) store
  NodeKin<Dual> kin;
  kin.vst = st;
  kin.dst = st + 1;
  kin.vstride = kin.dstride = 2;
  double sh[PL_ABA_SH];
  if (fam == PL_JF_ABA) {
    double raw[PL_ABA_RAW], kd[PL_KIN_STORE];
    NodeKin<double> kp;
    kp.store = kd;
    kp.stride = 1;
    for (int c = 0; c < M.nv + 2; ++c) aba_point_column(M, O, in0, in1, in3, c, kp, raw + c * M.nv);
    aba_factor_solve(M.nv, in2, raw, sh);
  }
  for (int col = 0; col < W; ++col) {
    int k, c;
    dyn_jac_locate(tan_len, wrt, col, &k, &c);
    double* out = jac + col;
    switch (fam) {
      case PL_JF_TREE: dyn_jac_column<PL_JF_TREE>(M, O, F, fn, flags, in0, in1, in2, in3, k, c, kin, sh, out, W); break;
      case PL_JF_COMP: dyn_jac_column<PL_JF_COMP>(M, O, F, fn, flags, in0, in1, in2, in3, k, c, kin, sh, out, W); break;
      case PL_JF_ABA: dyn_jac_column<PL_JF_ABA>(M, O, F, fn, flags, in0, in1, in2, in3, k, c, kin, sh, out, W); break;
      case PL_JF_CEN: dyn_jac_column<PL_JF_CEN>(M, O, F, fn, flags, in0, in1, in2, in3, k, c, kin, sh, out, W); break;
      case PL_JF_FRAME: dyn_jac_column<PL_JF_FRAME>(M, O, F, fn, flags, in0, in1, in2, in3, k, c, kin, sh, out, W); break;
      default: break;
    }
  }
}

}  // namespace pl
