// OSQP adaptive rho (host+device, fp64): the estimate and the update decision of one problem.
//
// Restates OSQP 0.6.x compute_rho_estimate / adapt_rho (src/auxil.c) on the solver's SCALED
// quantities (no E^-1, D^-1 or c^-1), all norms infinity norms:
//   nrm[0..2] = |A x - z|, |z|, |A x|
//   nrm[3..6] = |P x + q + A^T y|, |q|, |A^T y|, |P x|
//   pri = nrm[0] / (max(nrm[1], nrm[2]) + 1e-10)
//   dua = nrm[3] / (max(nrm[4], nrm[5], nrm[6]) + 1e-10)
//   rho_est = clip(rho sqrt(pri / (dua + 1e-10)), PL_RHO_MIN, PL_RHO_MAX)
//   update iff rho_est > rho tol or rho_est < rho / tol (both false for a non-finite estimate)
// The interval is a fixed number of iterations (a multiple of check_termination): OSQP's
// automatic interval is a fraction of the measured setup time, which is not deterministic, and
// is not restated.
// One definition for k_rho_adapt (k_rho.hip) and the host (pl_osqp_rho_estimate_host).
#pragma once
#include "ad.h"
#include "state.h"

namespace pl {

// rho of one row by OSQP's classes, from its scaled bounds (the rule of k_qp_finish)
PL_HD double rho_row(double lsr, double usr, double rho) {
  if (lsr < -PL_OSQP_INFTY * PL_MIN_SCALING && usr > PL_OSQP_INFTY * PL_MIN_SCALING) return PL_RHO_MIN;
  if (usr - lsr < PL_RHO_TOL) return PL_RHO_EQ_OVER_INEQ * rho;
  return rho;
}

// max that keeps a NaN operand (fmax would drop it): a NaN norm must reach the estimate
PL_HD double rho_nmax(double a, double b) { return (a > b || a != a) ? a : b; }

PL_HD double rho_estimate(const double* nrm, double rho) {
  const double pri = nrm[0] / (rho_nmax(nrm[1], nrm[2]) + 1e-10);
  const double dua = nrm[3] / (rho_nmax(nrm[4], rho_nmax(nrm[5], nrm[6])) + 1e-10);
  const double est = rho * sqrt(pri / (dua + 1e-10));
  // comparisons, not fmin / fmax: a NaN estimate stays NaN
  return est < PL_RHO_MIN ? PL_RHO_MIN : (est > PL_RHO_MAX ? PL_RHO_MAX : est);
}

PL_HD bool rho_update(double est, double rho, double tol) { return est > rho * tol || est < rho / tol; }

}  // namespace pl
