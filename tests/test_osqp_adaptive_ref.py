"""The adaptive-rho reference (tests/osqp_adaptive_ref.py) on small random QPs (CPU).

The only independent pin of the rule available without OSQP itself: with the option off the
reference is OSQPRef bit for bit; with it on, a strictly convex QP started from a badly
chosen rho updates rho, still lands on the QP's solution and meets the eps it was asked for.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.osqp_ref import REFERENCE_SETTINGS, SOLVED, OSQPRef
from osqp_adaptive_ref import OSQPAdaptiveRef

N_VAR, M_ROW = 12, 18


def random_qp(seed):
    """min 1/2 x'Px + q'x, l <= Ax <= u with P diagonal > 0; equality, two-sided, one-sided and
    free rows (the three rho classes)."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.5, 2.0, N_VAR)
    A = sp.random(M_ROW, N_VAR, density=0.4, random_state=seed, data_rvs=lambda k: rng.normal(size=k)).tolil()
    for r in range(M_ROW):  # no empty row
        A[r, r % N_VAR] = 1.0 + rng.uniform()
    A = A.tocsc()
    A.sort_indices()
    q = rng.normal(size=N_VAR)
    x0 = rng.normal(size=N_VAR)
    c = A @ x0
    l, u = c - rng.uniform(0.1, 1.0, M_ROW), c + rng.uniform(0.1, 1.0, M_ROW)
    l[:4] = u[:4] = c[:4]        # equalities
    l[4:7] = -np.inf              # one-sided
    l[7], u[7] = -np.inf, np.inf  # free
    return P, q, A, l, u


def make(cls, P, A, kkt, **over):
    s = dict(REFERENCE_SETTINGS)
    s.update(over)
    return cls(P, A, s, kkt=kkt, blocks=[(0, N_VAR, N_VAR)])


@pytest.mark.parametrize("kkt", ["quasi_definite", "reduced_block"])
def test_off_is_osqp_ref(kkt):
    P, q, A, l, u = random_qp(3)
    a, b = make(OSQPRef, P, A, kkt), make(OSQPAdaptiveRef, P, A, kkt)
    for k in range(3):  # warm-started repeats with changed data
        xa, ia = a.update_and_solve(q + 0.1 * k, A.data * (1 + 0.01 * k), l, u)
        xb, ib = b.update_and_solve(q + 0.1 * k, A.data * (1 + 0.01 * k), l, u)
        assert np.array_equal(xa, xb)
        assert (ia["status"], ia["iter"]) == (ib["status"], ib["iter"])
        assert ia["pri_res"] == ib["pri_res"] and ia["dua_res"] == ib["dua_res"]
        assert np.array_equal(a.y, b.y) and np.array_equal(a.z, b.z)
    assert b.decisions == [] and b.rho_b == REFERENCE_SETTINGS["rho"]


@pytest.mark.parametrize("kkt", ["quasi_definite", "reduced_block"])
@pytest.mark.parametrize("rho0", [1e-4, 1e2])
def test_adaptive_updates_and_converges(kkt, rho0):
    P, q, A, l, u = random_qp(5)
    eps = 1e-6
    exact = make(OSQPRef, P, A, kkt, rho=0.1, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
    xs, ist = exact.update_and_solve(q, A.data, l, u)
    assert ist["status"] == SOLVED
    ad = make(OSQPAdaptiveRef, P, A, kkt, rho=rho0, eps_abs=eps, eps_rel=eps, max_iter=20000, adaptive_rho=True)
    xa, ia = ad.update_and_solve(q, A.data, l, u)
    nupd = sum(1 for d in ad.decisions if d[3])
    print(f"rho0 {rho0} {kkt}: iters {ia['iter']}, updates {nupd}, rho_b {ad.rho_b:.3e}, "
          f"|x - x*| {np.abs(xa - xs).max():.2e}")
    assert nupd >= 1 and ad.rho_b != rho0
    # every update leaves the band, and the log is consistent with rho_b
    for it, rho, est, upd in ad.decisions:
        assert it % 25 == 0 and upd == (est > 5 * rho or est < rho / 5)
    assert ia["status"] == SOLVED
    # the eps it was asked for, recomputed from the returned point alone: the primal residual
    # of z = clip(Ax) and the termination bound eps (1 + max(|Ax|, |z|))
    Ax = A @ xa
    z = np.clip(Ax, l, u)
    assert np.abs(Ax - z).max() <= eps * (1 + max(np.abs(Ax).max(), np.abs(z).max()))
    # the solution: P >= 0.5 I makes the QP 0.5-strongly convex, so a point whose residuals are
    # O(eps (1 + data norms)) lies within O(eps) * (data norms ~ 10) / 0.5 of x*; 1e3 eps leaves a
    # factor ~50 for the constraint geometry
    assert np.abs(xa - xs).max() <= 1e3 * eps
    # the same problem with the fixed bad rho needs more iterations (what the option is for)
    fx = make(OSQPRef, P, A, kkt, rho=rho0, eps_abs=eps, eps_rel=eps, max_iter=20000)
    _, ifx = fx.update_and_solve(q, A.data, l, u)
    assert ia["iter"] <= ifx["iter"]


def test_rho_carries_over_and_resets():
    P, q, A, l, u = random_qp(7)
    ad = make(OSQPAdaptiveRef, P, A, "quasi_definite", rho=1e-4, adaptive_rho=True)
    ad.update_and_solve(q, A.data, l, u)
    r1 = ad.rho_b
    assert r1 != 1e-4
    ad.update_and_solve(q + 0.05, A.data, l, u)
    assert ad.decisions == [] or ad.decisions[0][1] == r1  # the second call started from r1
    ad.reset_rho()
    assert ad.rho_b == 1e-4


def test_update_at_max_iter_serves_the_next_call():
    """max_iter = one interval: the only decision is taken at it == max_iter, changes rho_b and
    leaves this call's iterates what the fixed-rho run gives."""
    P, q, A, l, u = random_qp(9)
    ad = make(OSQPAdaptiveRef, P, A, "quasi_definite", rho=1e-4, adaptive_rho=True, max_iter=25, eps_abs=1e-9,
              eps_rel=1e-9)
    fx = make(OSQPRef, P, A, "quasi_definite", rho=1e-4, max_iter=25, eps_abs=1e-9, eps_rel=1e-9)
    xa, ia = ad.update_and_solve(q, A.data, l, u)
    xf, _ = fx.update_and_solve(q, A.data, l, u)
    assert [d[0] for d in ad.decisions] == [25] and ad.decisions[0][3]
    assert np.array_equal(xa, xf) and ad.rho_b == ad.decisions[0][2]
