"""The two operand paths of the "sweep" ADMM kernel (pl_ocp_set_admm_operands) on the MI355X.

"fused" (default) skips the prefetches a step does not consume and computes rho from the row
bounds where k_qp_finish wrote it; "split" is the earlier path.  The arithmetic is the same, so
every case runs both with the sweep kernel forced and asserts bit equality (np.array_equal) of
step, x, za, ya, status and ADMM iteration count.

rho classes.  k_qp_finish writes PL_RHO_MIN for a row with both bounds infinite, 1e3 rho for an
equality row and rho otherwise.  Every OSQP case asserts that d.rho is exactly that rule applied
to the stored ls, us (what the fused kernel recomputes) and that the equality and the box class
both occur.  None of the fixtures has a row with both bounds infinite (the oracle's bounds of
sqp_go2_rnea_n20: 1380 equality, 652 box or one-sided rows, 0 unbounded; synthetic Go2 rnea
N = 2 / 3: 180 / 258 equality, 64 / 108 box, 0 unbounded), so the PL_RHO_MIN class is covered
by one more case: the N = 3 problem with two joint-velocity limits set to infinity, whose
-inf <= v_j <= inf rows are unbounded (4 rows by the oracle's bounds); that case asserts all
three classes.
"""
import numpy as np
import pytest

from conftest import golden, make_robot
from test_gpu import _batched

pytestmark = pytest.mark.gpu

RHO = 2e-2  # pinoloco.ocp.OSQP_SETTINGS["rho"]
MODES = ("split", "fused")


def _state(bo, st):
    B = bo.batch
    return {"step": bo.get_step(), "x": bo.get_x(), "za": bo.debug("za", B * bo.m).reshape(B, bo.m),
            "ya": bo.debug("ya", B * bo.m).reshape(B, bo.m), "status": np.array(st["status"]),
            "admm_iters": np.array(st["admm_iters"])}


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.all(np.isfinite(a["x"])) and np.all(np.isfinite(a["za"])), what


def _assert_rho(bo, unbounded):
    """d.rho is k_qp_finish's rule on the stored bounds, and the classes the case must have occur."""
    B, m = bo.batch, bo.m
    rho, ls, us = (bo.debug(k, B * m).reshape(B, m) for k in ("rho", "ls", "us"))
    unb = (ls < -1e30 * 1e-4) & (us > 1e30 * 1e-4)
    eq = ~unb & (us - ls < 1e-4)
    want = np.where(unb, 1e-6, np.where(eq, 1e3 * RHO, RHO))
    assert np.array_equal(rho, want)
    for b in range(B):
        assert eq[b].any() and (~unb[b] & ~eq[b]).any(), b
        if unbounded:
            assert unb[b].any(), b


def _synthetic(N, B, inf_limits=False, settings=None):
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    R = make_robot("go2")
    if inf_limits:
        R.joint_vel_max = np.array(R.joint_vel_max, dtype=np.float64)
        R.joint_vel_max[[1, 7]] = np.inf
    lay, P, X, XS, T0 = build_batch(R, "whole_body_rnea", N, B, 0)
    bo = BatchedOCP(R, "whole_body_rnea", N, batch=B, device=0, osqp_settings=settings)
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    return bo


def _solve_both(make, what, unbounded=False):
    out = {}
    for mode in MODES:
        bo = make()
        bo.set_admm_kernel("sweep")
        bo.set_admm_operands(mode)
        assert bo.admm_kernel() == "sweep" and bo.admm_operands() == mode
        st = bo.solve()
        assert bo.admm_rho_from_bounds() == (mode == "fused")
        _assert_rho(bo, unbounded)
        out[mode] = _state(bo, st)
        bo.close()
    _assert_same(out["split"], out["fused"], what)
    return out["fused"]


@pytest.mark.parametrize("B", [1, 5])
def test_golden_go2_rnea(B):
    """One problem per workgroup (PPW = 1), B = 5: a grid of several workgroups."""
    G = golden("sqp_go2_rnea_n20.npz")
    _solve_both(lambda: _batched("go2", "whole_body_rnea", 20, G, B=B)[1], B)


@pytest.mark.parametrize("N", [2, 3])
def test_shortest_horizons(N):
    """N = 2, 3: TN and T0 are adjacent, where the skipped-prefetch turn-around could fail."""
    _solve_both(lambda: _synthetic(N, 3), N)


def test_ragged_last_workgroup_and_batch_invariance():
    """B = 1027: four problems per workgroup, the last one with three idle waves; problem 0
    gives the same bits as alone."""
    big = _solve_both(lambda: _synthetic(3, 1027), 1027)
    one = _solve_both(lambda: _synthetic(3, 1), 1)
    for k in big:
        assert np.array_equal(big[k][0], one[k][0]), k


@pytest.mark.parametrize("ct", [10, 0])
def test_launch_lengths(ct):
    """max_iter 25 with check_termination 10 (launches of 10, 10, 5 iterations) and 0 (one launch
    of 25): launches of unequal length and a single launch."""
    G = golden("sqp_go2_rnea_n20.npz")
    from pinoloco.ocp import BatchedOCP

    def make():
        R = make_robot("go2", str(G["gait"]))
        bo = BatchedOCP(R, "whole_body_rnea", 20, batch=5, device=0, gait_type=str(G["gait"]),
                        osqp_settings={"max_iter": 25, "check_termination": ct})
        bo.set_params(G["P"][:5])
        bo.set_x(G["X"][:5])
        bo.init_solver()
        return bo

    out = _solve_both(make, ct)
    assert np.all(out["admm_iters"] <= 25)


def test_three_mpc_steps_with_graph_replay():
    """Every solve after the first starts from iterates other kernels wrote (warm start shift,
    rescaling), and the second and third steps run as graph replays."""
    G = golden("sqp_go2_rnea_n20.npz")
    out = {}
    for mode in MODES:
        R, bo = _batched("go2", "whole_body_rnea", 20, G, B=5)
        bo.set_admm_kernel("sweep")
        bo.set_admm_operands(mode)
        bo.mpc_setup(G["XS"][:5], G["T0"][:5])
        steps = []
        for k in range(3):
            bo.mpc_step(k)
            s = _state(bo, bo.mpc_stats())
            s["state"] = bo.mpc_state()
            steps.append(s)
            _assert_rho(bo, False)
        gi = bo.mpc_graph_info()
        assert gi["replays"] >= 1 and gi["eager_fallback"] == 0, gi
        out[mode] = steps
        bo.close()
    for k in range(3):
        for key in out["split"][k]:
            assert np.array_equal(out["split"][k][key], out["fused"][k][key]), (k, key)


def test_all_three_rho_classes():
    """Two infinite joint-velocity limits give rows with both bounds infinite: PL_RHO_MIN,
    equality and box rows in every problem."""
    _solve_both(lambda: _synthetic(3, 3, inf_limits=True), "inf", unbounded=True)


def test_interior_point_streams_rho():
    """The interior point writes per-row weights into d.rho: the fused sweep streams them
    (rho-from-bounds off) and the solve is bit-equal to the split path."""
    from pinoloco.ocp import BatchedOCP
    G = golden("ip_go2_rnea_n20.npz")
    gait = str(G["gait"])
    out = {}
    for mode in MODES:
        R = make_robot("go2", gait)
        bo = BatchedOCP(R, "whole_body_rnea", 20, batch=G["P"].shape[0], device=0, gait_type=gait)
        bo.set_solver("fatrop")
        bo.set_ip_settings()
        bo.set_admm_kernel("sweep")
        bo.set_admm_operands(mode)
        bo.set_params(G["P"])
        bo.set_x(G["X"])
        bo.init_solver()
        bo.solve()
        assert not bo.admm_rho_from_bounds()
        ips = bo.ip_stats()
        out[mode] = _state(bo, {"status": ips["status"], "admm_iters": ips["iter"]})
        out[mode]["lam"] = bo.get_lam()
        bo.close()
    for k in out["split"]:
        assert np.array_equal(out["split"][k], out["fused"][k]), k
    assert np.all(np.isfinite(out["fused"]["x"]))
