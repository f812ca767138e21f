"""OSQP adaptive rho on the GPU (pl_ocp_set_adaptive_rho) against the CPU reference
(tests/osqp_adaptive_ref.py through tests/golden/make_golden_adaptive.py, kkt="reduced_block").

Solve parity, per fixture and ADMM kernel: status, ADMM iterations, the number of rho updates
and the iteration of each exact; rho and the last estimate <= 1e-5 relative (the iterates agree
to ~1e-9 absolute on residuals that are above eps = 1e-3 when a decision is taken, through a
scaled A whose rows hold at most a few dozen entries of magnitude <= 1); the step dx at the bar
tests/test_gpu.py holds for the same shapes with a fixed rho (1e-9 relative), or ten times the
fixture's stored CPU-to-CPU gap (quasi_definite against reduced_block) where that is larger.
The measured maxima go to adaptive_rho_parity.json in the directory PL_TEST_OUT names (default:
test_out/ in the repository root); profiles/adaptive_rho/parity.json is a copy of one run.
"""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, golden, make_robot

pytestmark = pytest.mark.gpu

FIXTURES = [("adaptive_go2_rnea_n20", "go2", "whole_body_rnea", 20),
            ("adaptive_go2_cv_n20", "go2", "centroidal_vel", 20),
            ("adaptive_go2_rnea_n20_rho2e-4", "go2", "whole_body_rnea", 20)]
KERNELS = ("sweep", "sweep2", "chain")
OUT = os.path.join(os.environ.get("PL_TEST_OUT") or os.path.join(ROOT, "test_out"), "adaptive_rho_parity.json")
RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_records():
    yield
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(RECORDS, f, indent=1, sort_keys=True)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _handle(G, rname, dyn, N, P=None, X=None, adaptive=True, kernel=None, debug_paths=()):
    from pinoloco.ocp import BatchedOCP
    P = G["P"] if P is None else P
    X = G["X"] if X is None else X
    bo = BatchedOCP(make_robot(rname), dyn, N, batch=P.shape[0], device=0, osqp_settings={"rho": float(G["rho"])},
                    gait_type="trot", debug_paths=debug_paths)
    if adaptive:
        bo.set_adaptive_rho(True, int(G["interval"]), float(G["tolerance"]))
    if kernel:
        bo.set_admm_kernel(kernel)
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    return bo


def _updates(dec):
    """Iterations of the updates in one solve's decision log ([K][4], NaN padded)."""
    return [int(d[0]) for d in dec if d[3] == 1.0]


def _check_rho(bo, decs, rho_b, tag):
    """Update counts and iterations exact, rho and the last estimate <= 1e-5; returns the errors.
    A solve without a decision leaves the estimate what it was: not compared then."""
    r = bo.osqp_rho()
    its = bo.debug("rho_upd_it", bo.batch * 8).reshape(bo.batch, 8)
    errs = []
    for b in range(bo.batch):
        want = _updates(decs[b])
        assert r["updates"][b] == len(want), (tag, b, r["updates"][b], want)
        assert [int(v) for v in its[b] if v > 0] == want, (tag, b)
        taken = [d for d in decs[b] if not np.isnan(d[0])]
        e = (abs(r["rho"][b] / rho_b[b] - 1.0), abs(r["rho_estimate"][b] / taken[-1][2] - 1.0) if taken else 0.0)
        errs.append(e)
        assert max(e) <= 1e-5, (tag, b, e)
    return errs


def test_fixtures_show_what_the_tests_need():
    """Re-asserted from the stored decision logs: a problem with mid-solve updates, a problem
    with none in its solve (in a fixture that also has an updating one: the mask), an update at
    it == max_iter that the next solve of the loop starts from, no decision within 1 % of a
    threshold."""
    mid = quiet_beside_mid = last = False
    for name, *_ in FIXTURES:
        G = golden(f"{name}.npz")
        tol, mi = float(G["tolerance"]), int(G["osqp_max_iter"])
        logs = [G["dec"]] + ([G["loop_dec"]] if "loop_dec" in G else [])
        for d in np.concatenate([x.reshape(-1, 4) for x in logs]):
            if not np.isnan(d[0]):
                assert abs(d[2] / (d[1] * tol) - 1) > 0.01 and abs(d[2] / (d[1] / tol) - 1) > 0.01, (name, d)
                assert bool(d[3]) == (d[2] > d[1] * tol or d[2] < d[1] / tol)
        m = [b for b in range(4) if any(i < mi for i in _updates(G["dec"][b]))]
        q = [b for b in range(4) if not _updates(G["dec"][b])]
        mid |= bool(m)
        quiet_beside_mid |= bool(m and q)
        if "loop_dec" in G:
            for b in range(G["loop_dec"].shape[0]):
                for k in range(G["loop_dec"].shape[1] - 1):
                    if mi in _updates(G["loop_dec"][b, k]):
                        assert G["loop_dec"][b, k + 1][0][1] == G["loop_rho_b"][b, k]
                        last = True
    assert mid and quiet_beside_mid and last


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name,rname,dyn,N", FIXTURES)
def test_solve_parity(name, rname, dyn, N, kernel):
    G = golden(f"{name}.npz")
    bo = _handle(G, rname, dyn, N, kernel=kernel)
    assert bo.admm_kernel() == kernel and not bo.admm_rho_from_bounds()
    st = bo.solve()
    dx = bo.get_step()
    bar = max(1e-9, 10.0 * float(G["dx_gap"].max()))
    rec = {"dx_rel": [], "dx_bar": bar, "rho_rel": [], "rho_estimate_rel": []}
    try:
        for b in range(bo.batch):
            assert st["status"][b] == G["status"][b] and st["admm_iters"][b] == G["iters"][b], (b, st)
        errs = _check_rho(bo, G["dec"], G["rho_b"], name)
        rec["rho_rel"], rec["rho_estimate_rel"] = [e[0] for e in errs], [e[1] for e in errs]
        rec["dx_rel"] = [_rel(dx[b], G["dx"][b]) for b in range(bo.batch)]
        print(name, kernel, "dx", rec["dx_rel"], "bar", bar, "rho", rec["rho_rel"], rec["rho_estimate_rel"])
        assert max(rec["dx_rel"]) < bar, rec
        for b in range(bo.batch):  # the line search ran on that step
            assert [st["ls_accepted"][b], st["ls_branch"][b], st["ls_trials"][b]] == \
                [G["accepted"][b], G["branch"][b], G["trials"][b]], b
    finally:
        RECORDS[f"{name}/{kernel}"] = rec
        bo.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_off_means_untouched(kernel):
    """Never set / set on / set off again on one handle: the first and the third solve are the
    same bits, and the off handle computes rho from the bounds as before."""
    name, rname, dyn, N = FIXTURES[0]
    G = golden(f"{name}.npz")
    bo = _handle(G, rname, dyn, N, adaptive=False, kernel=kernel)

    def run():
        bo.set_x(G["X"])
        bo.init_solver()
        st = bo.solve()
        return bo.get_x(), bo.get_step(), st

    x1, s1, st1 = run()
    assert bo.admm_rho_from_bounds()
    assert bo.osqp_rho()["updates"].tolist() == [0] * 4 and np.all(bo.osqp_rho()["rho"] == float(G["rho"]))
    bo.set_adaptive_rho(True)
    assert not bo.admm_rho_from_bounds()
    x2, _, st2 = run()
    assert bo.osqp_rho()["updates"].sum() > 0 and not np.array_equal(x1, x2)
    assert not bo.admm_rho_from_bounds()
    bo.set_adaptive_rho(False)
    x3, s3, st3 = run()
    assert bo.admm_rho_from_bounds()
    assert np.array_equal(x1, x3) and np.array_equal(s1, s3)
    for key in ("status", "admm_iters", "pri_res", "dua_res", "ls_alpha", "f", "viol_max"):
        assert np.array_equal(st1[key], st3[key]), key
    assert bo.osqp_rho()["updates"].tolist() == [0] * 4
    bo.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_mask_leaves_quiet_neighbours_alone(kernel):
    """Problem 0 updates and is refactored mid-solve; problems 1..3 are copies of a problem that
    never updates: their x is the bits a batch of one gives, so a neighbour's refactor and rhs
    rebuild do not touch them."""
    name, rname, dyn, N = FIXTURES[1]
    G = golden(f"{name}.npz")
    quiet = [b for b in range(4) if not _updates(G["dec"][b])][0]
    loud = [b for b in range(4) if any(i < 100 for i in _updates(G["dec"][b]))][0]
    idx = [loud, quiet, quiet, quiet]
    bo = _handle(G, rname, dyn, N, P=G["P"][idx], X=G["X"][idx], kernel=kernel)
    bo.solve()
    x4, s4, r4 = bo.get_x(), bo.get_step(), bo.osqp_rho()
    bo.close()
    assert r4["updates"].tolist() == [len(_updates(G["dec"][loud])), 0, 0, 0]
    b1 = _handle(G, rname, dyn, N, P=G["P"][[quiet]], X=G["X"][[quiet]], kernel=kernel)
    b1.solve()
    x1, s1 = b1.get_x(), b1.get_step()
    b1.close()
    for b in (1, 2, 3):
        assert np.array_equal(x4[b], x1[0]) and np.array_equal(s4[b], s1[0]), b
    assert _rel(s4[0], G["dx"][loud]) < max(1e-9, 10.0 * float(G["dx_gap"].max()))


def _loop(G, rname, dyn, N, debug_paths=()):
    bo = _handle(G, rname, dyn, N, debug_paths=debug_paths)
    bo.mpc_setup(G["XS"], G["T0"])
    states, rhos = [], []
    for k in range(G["loop_states"].shape[1]):
        bo.mpc_step(k)
        S = bo.mpc_state()
        st = bo.mpc_stats()
        for b in range(bo.batch):
            assert _rel(S[b], G["loop_states"][b, k]) < 1e-7, (k, b)
            assert [st["status"][b], st["admm_iters"][b], st["ls_branch"][b], st["ls_trials"][b]] == \
                G["loop_stats"][b, k].tolist(), (k, b)
        # rho carried from step to step: every solve starts from the previous one's rho_b
        _check_rho(bo, G["loop_dec"][:, k], G["loop_rho_b"][:, k], f"step {k}")
        states.append(S)
        rhos.append(bo.osqp_rho()["rho"])
    return bo, np.array(states), np.array(rhos)


def test_mpc_loop_carries_rho_and_replays():
    name, rname, dyn, N = FIXTURES[0]
    G = golden(f"{name}.npz")
    bo, S, rhos = _loop(G, rname, dyn, N)
    info = bo.mpc_graph_info()
    assert info == {"captures": 1, "replays": 3, "eager_fallback": 0}, info
    bo.set_adaptive_rho(True, 0, 6.0)  # a change of the settings: one eager step, one new capture
    bo.mpc_step(4)
    bo.mpc_step(5)
    bo.mpc_step(6)
    assert bo.mpc_graph_info() == {"captures": 2, "replays": 5, "eager_fallback": 0}
    bo.close()
    be, Se, rhose = _loop(G, rname, dyn, N, debug_paths=("no_mpc_graph",))
    assert be.mpc_graph_info()["captures"] == 0
    be.close()
    assert np.array_equal(S, Se) and np.array_equal(rhos, rhose)


def test_setter_is_inert_with_the_interior_point():
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    R = make_robot("go2")
    lay, P, X, XS, T0 = build_batch(R, "whole_body_rnea", 10, 2, 0)
    out = []
    for on in (False, True):
        bo = BatchedOCP(R, "whole_body_rnea", 10, batch=2, device=0)
        bo.set_solver("fatrop")
        bo.set_ip_settings()
        if on:
            bo.set_adaptive_rho(True, 25, 5.0)
            assert bo.adaptive_rho() == (True, 25, 5.0)
        bo.set_params(P)
        bo.set_x(X)
        bo.init_solver()
        bo.solve()
        out.append((bo.get_x(), bo.get_lam(), bo.ip_stats()["iter"]))
        bo.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
