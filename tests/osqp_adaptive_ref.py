"""Reference (test infrastructure) of OSQP's adaptive rho on top of oracle/osqp_ref.py.

``OSQPAdaptiveRef.update_and_solve`` restates ``OSQPRef.update_and_solve`` (the same
statements in the same order, so that with ``adaptive_rho`` off the results are the same
bits) and adds OSQP 0.6.x's rule (auxil.c compute_rho_estimate / adapt_rho, osqp.c
osqp_update_rho) as include/pinoloco.h states it:

* the solver holds ``rho_b`` (``settings->rho``), initialised to ``settings["rho"]`` and
  carried across calls;
* at iteration ``it`` with ``it % interval == 0`` (interval 0 = check_termination, else a
  multiple of it), after the termination check's exact pass left the problem unsolved --
  ``it == max_iter`` included, before the approximate pass -- on the SCALED quantities
      pri = |Ax - z| / (max(|z|, |Ax|) + 1e-10)
      dua = |Px + q + A'y| / (max(|q|, |A'y|, |Px|) + 1e-10)
      rho_est = clip(rho_b sqrt(pri / (dua + 1e-10)), 1e-6, 1e6)
  and iff rho_est > rho_b tol or rho_est < rho_b / tol: rho_b = rho_est, the row weights are
  rewritten by the classes (loose RHO_MIN, equality 1e3 rho_b, else rho_b) and the KKT matrix
  is refactored (both kkt modes); x, z, y stay.  At max_iter nothing is refactored.

``decisions`` lists ``(iteration, rho_before, rho_est, updated)`` of the last call.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.osqp_ref import (MAX_ITER_REACHED, MIN_SCALING, NON_CVX, OSQP_INFTY, DUAL_INFEASIBLE,
                             DUAL_INFEASIBLE_INACCURATE, PRIMAL_INFEASIBLE, PRIMAL_INFEASIBLE_INACCURATE, RHO_EQ_OVER_RHO_INEQ,
                             RHO_MIN, RHO_TOL, UNSOLVED, BlockReduced, OSQPRef, _inf_norm)

RHO_MAX = 1e6


def rho_estimate(norms, rho):
    """The estimate from the seven scaled norms (|Ax - z|, |z|, |Ax|, |Px + q + A'y|, |q|, |A'y|, |Px|)."""
    with np.errstate(all="ignore"):
        pri = np.float64(norms[0]) / (max(norms[1], norms[2]) + 1e-10)
        dua = np.float64(norms[3]) / (max(norms[4], norms[5], norms[6]) + 1e-10)
        est = rho * np.sqrt(pri / (dua + 1e-10))
    return float(min(max(est, RHO_MIN), RHO_MAX))


def rho_update(est, rho, tol):
    return bool(est > rho * tol or est < rho / tol)


class OSQPAdaptiveRef(OSQPRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rho_b = float(self.s["rho"])
        self.decisions = []

    def reset_rho(self):
        self.rho_b = float(self.s["rho"])

    def _rho_vec(self, ls, us, rho_b):
        rho = np.full(self.m, rho_b)
        loose = (ls < -OSQP_INFTY * MIN_SCALING) & (us > OSQP_INFTY * MIN_SCALING)
        eq = (~loose) & (us - ls < RHO_TOL)
        rho[loose] = RHO_MIN
        rho[eq] = RHO_EQ_OVER_RHO_INEQ * rho_b
        return rho

    def update_and_solve(self, q, Ax, l, u):
        s = self.s
        adaptive = bool(s.get("adaptive_rho", False))
        interval = int(s.get("adaptive_rho_interval", 0)) or int(s["check_termination"] or 0)
        tol = float(s.get("adaptive_rho_tolerance", 5.0))
        n, m = self.n, self.m
        A_raw = sp.csc_matrix((np.asarray(Ax, dtype=float), self.A_pat.indices, self.A_pat.indptr),
                              shape=self.A_pat.shape)
        l = np.maximum(np.asarray(l, dtype=float), -OSQP_INFTY)
        u = np.minimum(np.asarray(u, dtype=float), OSQP_INFTY)
        P, qs, A, D, E, c = self._scale(self.P_raw, np.asarray(q, dtype=float), A_raw)
        Dinv, Einv, cinv = 1.0 / D, 1.0 / E, 1.0 / c
        ls, us = E * l, E * u
        self.scaling = (D, E, c)
        rho = self._rho_vec(ls, us, self.rho_b if adaptive else s["rho"])
        rho_inv = 1.0 / rho
        sigma, alpha = s["sigma"], s["alpha"]

        def factor(rho, rho_inv):
            if self.kkt == "quasi_definite":
                KKT = sp.bmat([[sp.diags(P + sigma), A.T], [A, sp.diags(-rho_inv)]], format="csc")
                return spla.splu(KKT, permc_spec="COLAMD"), None
            return None, BlockReduced(sp.diags(P + sigma) + A.T @ sp.diags(rho) @ A, self.blocks, self.S_override)

        lu, red = factor(rho, rho_inv)
        x, z, y = self.x.copy(), self.z.copy(), self.y.copy()
        if not s["warm_start"]:
            x[:], z[:], y[:] = 0, 0, 0
        status = UNSOLVED
        it_done = 0
        info = {}
        delta_x = np.zeros(n)
        delta_y = np.zeros(m)
        can_check = False
        self.decisions = []

        def adapt(it, info):
            """True when rho_b changed."""
            norms = [_inf_norm(info["Ax"] - info["z"]), _inf_norm(info["z"]), _inf_norm(info["Ax"]),
                     _inf_norm(info["Px"] + info["q"] + info["Aty"]), _inf_norm(info["q"]), _inf_norm(info["Aty"]),
                     _inf_norm(info["Px"])]
            est = rho_estimate(norms, self.rho_b)
            upd = rho_update(est, self.rho_b, tol)
            self.decisions.append((it, self.rho_b, est, upd))
            if upd:
                self.rho_b = est
            return upd

        for it in range(1, s["max_iter"] + 1):
            x_prev, z_prev = x, z
            if self.kkt == "quasi_definite":
                rhs = np.concatenate([sigma * x_prev - qs, z_prev - rho_inv * y])
                sol = lu.solve(rhs)
                xt = sol[:n]
                zt = (z_prev - rho_inv * y) + rho_inv * sol[n:]
            else:
                xt = red.solve(sigma * x_prev - qs + A.T @ (rho * z_prev - y))
                zt = A @ xt
            x = alpha * xt + (1 - alpha) * x_prev
            delta_x = x - x_prev
            z = np.clip(alpha * zt + (1 - alpha) * z_prev + rho_inv * y, ls, us)
            delta_y = rho * (alpha * zt + (1 - alpha) * z_prev - z)
            y = y + delta_y
            it_done = it
            can_check = s["check_termination"] and it % s["check_termination"] == 0
            if can_check:
                info = self._info(P, qs, A, x, z, y, Dinv, Einv, cinv)
                status = self._check(info, P, qs, A, ls, us, delta_x, delta_y, D, Dinv, Einv, c, cinv, False)
                if status != UNSOLVED:
                    break
                if adaptive and interval and it % interval == 0 and adapt(it, info) and it < s["max_iter"]:
                    rho = self._rho_vec(ls, us, self.rho_b)
                    rho_inv = 1.0 / rho
                    lu, red = factor(rho, rho_inv)
        if not can_check:
            info = self._info(P, qs, A, x, z, y, Dinv, Einv, cinv)
            status = self._check(info, P, qs, A, ls, us, delta_x, delta_y, D, Dinv, Einv, c, cinv, False)
            if status == UNSOLVED and adaptive and interval and it_done % interval == 0:
                adapt(it_done, info)
        if status == UNSOLVED:
            st2 = self._check(info, P, qs, A, ls, us, delta_x, delta_y, D, Dinv, Einv, c, cinv, True)
            status = st2 if st2 != UNSOLVED else MAX_ITER_REACHED
        info["iter"] = it_done
        info["status"] = status
        if status in (PRIMAL_INFEASIBLE, PRIMAL_INFEASIBLE_INACCURATE, DUAL_INFEASIBLE,
                      DUAL_INFEASIBLE_INACCURATE, NON_CVX):
            sol_x = np.full(n, np.nan)
            self.x[:], self.z[:], self.y[:] = 0, 0, 0
        else:
            sol_x = D * x
            self.x, self.z, self.y = x, z, y
        return sol_x, info
