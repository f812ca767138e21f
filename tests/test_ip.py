"""Interior-point path (the reference's Fatrop branch, ocp.py:248-263 / 360-373) against
the numpy restatement oracle/ip_ref.py and its golden vectors tests/golden/ip_*.npz, with
the exact Lagrangian Hessian and the inertia correction (the default, pl_ip_settings.hessian).

Fatrop itself is not available here (PARITY UNPINNED against it); the restatement fixes
the algorithm, and the GPU path must reproduce it:

* per problem: termination status and iteration count exact, the accepted steps of
  the 10 iterations, the returned iterate x and the multipliers lam_g <= 1e-7 relative
  (inf-norm over the problem).  Measured on the MI355X with the exact Hessian
  (profiles/r03i/ip_parity_*.json): x <= 4.1e-9, lam <= 2.1e-9, steps <= 1.3e-8 on every
  fixture problem, the cold centroidal_vel starts included;
* teacher forcing: every iteration's Newton direction (dx, dlam, ds) and step bounds
  from the oracle's own iterate <= 1e-8 (measured <= 4.5e-9,
  profiles/r03i/ip_forced_*.json);  The GPU solves the reduced Newton
  system with the block-inverse factor of the OSQP branch (equality rows weighted
  1 / delta_c = 1e4) plus two refinement solves, the oracle with a sparse LU; one
  Newton direction agrees to ~1e-12 and the nonlinear iteration carries that
  through 10 steps;
* the 3-step closed loop (warm start incl. lam_g -> IP solve -> integrate) on the device:
  states <= 1e-6 relative; a solve warm-started from given multipliers (pl_ocp_set_lam)
  against the oracle's warm start;
* the CPU tests pin the restatement itself: the feasible standing problem converges
  (status 1) in a few iterations to the KKT tolerance, and the oracle reproduces its
  own fixture.
"""
import json
import os

import numpy as np
import pytest

from conftest import golden, make_robot

IP_FIXTURES = [("ip_go2_rnea_n20", "go2", "whole_body_rnea", 20), ("ip_go2_rnea_n20_stand", "go2", "whole_body_rnea", 20),
               ("ip_go2_cv_n20", "go2", "centroidal_vel", 20), ("ip_b2_aba_n40", "b2", "whole_body_aba", 40),
               ("ip_b2g_acc_n50", "b2g", "whole_body_acc", 50), ("ip_b2g_rnea_n50", "b2g", "whole_body_rnea", 50),
               ("ip_go2_cv_n20_stand", "go2", "centroidal_vel", 20), ("ip_go2_cv_nb_n20", "go2", "centroidal_vel", 20),
               ("ip_go2_ca_n20", "go2", "centroidal_acc", 20), ("ip_go2_acc_nb_n20", "go2", "whole_body_acc", 20)]
HERE = os.path.dirname(os.path.abspath(__file__))
# Problems whose trajectories would be checked by teacher forcing only.  With the
# Gauss-Newton Hessian (r02) the two cold centroidal_vel starts amplified 1e-12 differences
# of the directions into other filter decisions; with the exact Lagrangian Hessian (r03)
# every fixture trajectory, those included, agrees to <= 1.3e-8, so none is excluded.
CHAOTIC = set()
# Teacher-forced direction tolerance (relative, inf-norm): 1e-8 everywhere (the r02
# exceptions for ill-conditioned iterations of the cold starts measure <= 1e-10 now).
TF_TOL = {}
# Fixtures whose every problem is chaotic (none)
TRAJ_EXCLUDED = set()
TRAJ_TOL = 1e-7  # accepted steps, x and lam after the 10 iterations (relative, inf-norm)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def test_ip_oracle_converges_at_stand():
    """From the static standing equilibrium (feasible start) the restated IP converges in a
    few Newton steps, as an interior point must (status 1, error <= tol)."""
    G = golden("ip_go2_rnea_n20_stand.npz")
    assert int(G["status"][0]) == 1 and int(G["iter"][0]) <= 8
    assert float(G["err"][0]) <= 1e-3
    assert float(G["viol_max"][0]) < 1e-3


def test_ip_oracle_reproduces_fixture():
    from oracle.ip_ref import IPRef
    from oracle.ocp import OracleOCP
    G = golden("ip_go2_rnea_n20_stand.npz")
    R = make_robot("go2", "stand")
    o = OracleOCP(R, "whole_body_rnea", 20)
    x, lam, st = IPRef(o).solve(G["X"][0], G["P"][0])
    assert st["status"] == int(G["status"][0]) and st["iter"] == int(G["iter"][0])
    assert _rel(x, G["x_out"][0]) < 1e-9
    assert _rel(lam, G["lam"][0]) < 1e-7


def test_ip_oracle_lam_warm_start():
    """lam_g warm start (ocp_whole_body_rnea.py:234-235): from the multipliers of the
    converged standing solve, the same problem restarts at the solution (status 1 within
    two iterations), and the multipliers of the slack bounds split by the sign of lam."""
    from oracle.ip_ref import IPRef
    from oracle.ocp import OracleOCP
    G = golden("ip_go2_rnea_n20_stand.npz")
    R = make_robot("go2", "stand")
    ip = IPRef(OracleOCP(R, "whole_body_rnea", 20))
    x, lam, st = ip.solve(G["x_out"][0], G["P"][0], lam0=G["lam"][0])
    assert st["status"] == 1 and st["iter"] <= 2
    t0 = ip.trace[0] if ip.trace else None
    if t0 is not None:
        lam0 = G["lam"][0]
        assert np.array_equal(t0["lam"], lam0)
        assert np.all(t0["zu"][lam0 > 1e-7] == lam0[lam0 > 1e-7])


# Warm-started solves of the benchmark's MPC loop at step 2 (make_golden.py ip_warm_fixture):
# the exit the benchmark sees on ~30 % of its problems, a failed filter line search (status -2,
# no restoration phase: the last iterate is returned, as opti.debug does, ocp.py:362-365)
IP_WARM_FIXTURES = [("ip_b2g_rnea_n50_warm", "b2g", "whole_body_rnea", 50),
                    ("ip_b2g_acc_n50_warm", "b2g", "whole_body_acc", 50)]


def test_ip_fixture_coverage():
    """The fixtures exercise convergence, the iteration limit, the failed line search, every
    dynamics family and fraction-to-boundary-limited steps (alpha < 1)."""
    st, dyns, alphas = [], set(), []
    for name, _, dyn, _ in IP_FIXTURES + IP_WARM_FIXTURES:
        G = golden(f"{name}.npz")
        st += [int(s) for s in G["status"]]
        dyns.add(dyn)
        alphas.append(np.asarray(G["alphas"]).ravel())
    assert 1 in st and -1 in st and -2 in st
    for name, *_ in IP_WARM_FIXTURES:  # each warm fixture holds both exits of the benchmark
        G = golden(f"{name}.npz")
        assert {-1, -2} <= set(int(s) for s in G["status"]) and G["P"].shape[0] >= 8, name
    assert dyns == {"whole_body_rnea", "whole_body_acc", "whole_body_aba", "centroidal_vel", "centroidal_acc"}
    # both forms of the base in u (include_base False: ocp_centroidal_vel.py:9-23, ocp_whole_body_acc.py:124-135)
    assert {int(golden(f"{n}.npz")["include_base"]) for n, *_ in IP_FIXTURES if "include_base" in golden(f"{n}.npz")} == {0, 1}
    # every trajectory fixture checks at least one problem (the chaotic cold starts are teacher-forced)
    for name, *_ in IP_FIXTURES:
        G = golden(f"{name}.npz")
        if name not in TRAJ_EXCLUDED:
            assert any((name, b) not in CHAOTIC for b in range(G["P"].shape[0])), name
    a = np.concatenate(alphas)
    assert np.any((a > 0) & (a < 1)) and np.any(a == 1)


def test_ip_settings_validation():
    from pinoloco import _lib
    from pinoloco.ocp import BatchedOCP, OCP
    R = make_robot("go2")
    bo = BatchedOCP(R, "whole_body_rnea", 20, batch=1, device=-1)
    bo.set_ip_settings()  # the reference's settings are accepted
    with pytest.raises(_lib.PinolocoError):
        bo.set_ip_settings(max_iter=100)
    with pytest.raises(_lib.PinolocoError):
        bo.set_ip_settings(tol=0.0)
    with pytest.raises(ValueError):
        bo.set_solver("ipopt")
    with pytest.raises(ValueError):
        OCP(R, "ipopt", 20, "whole_body_rnea", device=-1)
    bo.close()


def _run_batched(name, rname, dyn, N):
    from pinoloco.ocp import BatchedOCP
    G = golden(f"{name}.npz")
    gait = str(G["gait"])
    R = make_robot(rname, gait)
    B = G["P"].shape[0]
    ib = bool(int(G["include_base"])) if "include_base" in G else True
    bo = BatchedOCP(R, dyn, N, batch=B, device=0, gait_type=gait, include_base=ib)
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"])
    bo.set_x(G["X"])
    bo.init_solver()
    bo.solve()
    return G, bo, bo.get_x(), bo.get_lam(), bo.ip_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("name,rname,dyn,N", IP_FIXTURES)
def test_ip_gpu_matches_oracle(name, rname, dyn, N):
    """Errors are recorded for every problem (gpurun_out/ip_parity_*.json) and asserted for
    the problems outside CHAOTIC."""
    G, bo, X, LAM, st = _run_batched(name, rname, dyn, N)
    errs = []
    for b in range(G["P"].shape[0]):
        n_it = int(G["iter"][b])
        same = int(st["status"][b]) == int(G["status"][b]) and int(st["iter"][b]) == n_it
        errs.append(dict(problem=b, chaotic=(name, b) in CHAOTIC, same_outcome=bool(same),
                         x=_rel(X[b], G["x_out"][b]), lam=_rel(LAM[b], G["lam"][b]),
                         alphas=_rel(st["alphas"][b][:n_it], G["alphas"][b][:n_it]) if n_it else 0.0))
    os.makedirs(os.path.join(HERE, "..", "gpurun_out"), exist_ok=True)
    with open(os.path.join(HERE, "..", "gpurun_out", f"ip_parity_{name}.json"), "w") as f:
        json.dump(errs, f, indent=1)
    for e in errs:
        if e["chaotic"]:
            continue
        assert e["same_outcome"], e
        assert e["alphas"] <= TRAJ_TOL, e
        assert e["x"] <= TRAJ_TOL, e
        assert e["lam"] <= TRAJ_TOL, e
    bo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,rname,dyn,N", IP_WARM_FIXTURES)
def test_ip_gpu_warm_started_matches_oracle(name, rname, dyn, N):
    """The benchmark loop's step-2 solves (warm start x and lam_g from step 1) against the
    oracle: status (-2 included), iteration count and every accepted step exact / <= 1e-7, the
    returned iterate x and lam_g <= 1e-7 relative.  A failed solve records alpha 0 for its
    last iteration (ip_ref.py), the GPU the same."""
    from pinoloco.ocp import BatchedOCP
    G = golden(f"{name}.npz")
    B = G["P"].shape[0]
    bo = BatchedOCP(make_robot(rname, "trot"), dyn, N, batch=B, device=0, gait_type="trot")
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"])
    bo.set_x(G["X"])
    bo.init_solver()
    bo.set_lam(G["LAM0"])
    bo.solve()
    X, LAM, st = bo.get_x(), bo.get_lam(), bo.ip_stats()
    errs = []
    for b in range(B):
        n_it = int(G["iter"][b]) + (1 if int(G["status"][b]) == -2 else 0)  # incl. the failed iteration's 0
        errs.append(dict(problem=b, gidx=int(G["gidx"][b]), status=int(st["status"][b]),
                         status_oracle=int(G["status"][b]), iter=int(st["iter"][b]), iter_oracle=int(G["iter"][b]),
                         x=_rel(X[b], G["x_out"][b]), lam=_rel(LAM[b], G["lam"][b]),
                         alphas=_rel(st["alphas"][b][:n_it], G["alphas"][b][:n_it])))
    os.makedirs(os.path.join(HERE, "..", "gpurun_out"), exist_ok=True)
    with open(os.path.join(HERE, "..", "gpurun_out", f"ip_parity_{name}.json"), "w") as f:
        json.dump(errs, f, indent=1)
    for e in errs:
        assert (e["status"], e["iter"]) == (e["status_oracle"], e["iter_oracle"]), e
        assert e["alphas"] <= TRAJ_TOL and e["x"] <= TRAJ_TOL and e["lam"] <= TRAJ_TOL, e
    bo.close()


@pytest.mark.gpu
def test_ip_gpu_refinement_counts_and_gather_path():
    """The refinement of each Newton system (k_ip_refine): on the headline-shape fixture every
    system gets at least the first solve plus one correction, and more than two on average (a
    refinement that contracts at a rate in (0.5, 0.9) keeps going; it stops on stagnation
    > 0.9, on |correction| <= 1e-12 |dx|, or at n_refine = 8).  The per-problem solve counts are
    written to gpurun_out/ip_refine_counts.json and pinned below.  The per-column global gather
    of H_i dx (the path of node blocks wider than the LDS vectors, nw > 192; forced here by
    PL_PATH_IP_REFINE_GATHER) gives the same solve as the LDS path to round-off."""
    from pinoloco.ocp import BatchedOCP
    name = "ip_b2g_rnea_n50"
    G = golden(f"{name}.npz")
    B = G["P"].shape[0]
    out = {}
    for paths in ((), ("ip_refine_gather",)):
        bo = BatchedOCP(make_robot("b2g", "trot"), "whole_body_rnea", 50, batch=B, device=0, gait_type="trot",
                        debug_paths=paths)
        bo.set_solver("fatrop")
        bo.set_ip_settings()
        bo.set_params(G["P"])
        bo.set_x(G["X"])
        bo.init_solver()
        bo.solve()
        out[paths] = (bo.get_x(), bo.get_lam(), bo.ip_stats())
        bo.close()
    X, LAM, st = out[()]
    Xg, LAMg, stg = out[("ip_refine_gather",)]
    iters = st["iter"].astype(int)
    solves = st["ref_solves"].astype(int)
    os.makedirs(os.path.join(HERE, "..", "gpurun_out"), exist_ok=True)
    with open(os.path.join(HERE, "..", "gpurun_out", "ip_refine_counts.json"), "w") as f:
        json.dump({"iter": iters.tolist(), "ref_solves": solves.tolist(),
                   "ref_solves_gather": stg["ref_solves"].astype(int).tolist()}, f)
    assert np.all(solves >= 2 * iters) and np.all(solves <= 9 * iters)
    assert solves.sum() > 2 * iters.sum()
    if REFINE_COUNTS.get(name) is not None:
        assert solves.tolist() == REFINE_COUNTS[name]
    for b in range(B):
        assert (int(stg["status"][b]), int(stg["iter"][b])) == (int(st["status"][b]), int(st["iter"][b]))
        assert _rel(Xg[b], X[b]) < 1e-9 and _rel(LAMg[b], LAM[b]) < 1e-8
        assert _rel(X[b], G["x_out"][b]) < TRAJ_TOL


# linear solves per problem of the fixture's solve (first solves + refinement corrections),
# measured on the MI355X with the current refinement rule (gpurun_out/ip_refine_counts.json)
# (51 .. 52 per problem, profiles/r06/b/ip_refine_counts.json, until k_fnode's u sweep formed its
# pivot columns directly: the smaller residual of C^-1 lets every refinement stop after two corrections)
REFINE_COUNTS = {"ip_b2g_rnea_n50": [30, 30, 30, 30, 30, 30, 30, 30]}


@pytest.mark.gpu
def test_ip_gpu_closed_loop():
    """3 MPC steps of the device loop with the interior-point solver and lam_g carried (the Opti
    branch, pl_mpc_set_ip_lam(o, 1)) vs the oracle's loop."""
    from pinoloco.ocp import BatchedOCP
    G = golden("ip_go2_rnea_n20.npz")
    R = make_robot("go2", "trot")
    bo = BatchedOCP(R, "whole_body_rnea", 20, batch=1, device=0, gait_type="trot")
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"][:1])
    bo.set_x(G["X"][:1])
    bo.init_solver()
    bo.mpc_set_ip_lam(True)
    bo.mpc_setup(G["XS"][:1], G["T0"][:1])
    steps = G["loop_states"].shape[0]
    for k in range(steps):
        bo.mpc_step(k)
        st = bo.ip_stats()
        assert int(st["status"][0]) == int(G["loop_stats"][k][0])
        assert int(st["iter"][0]) == int(G["loop_stats"][k][1])
    xs = bo.mpc_state()[0]
    assert _rel(xs, G["loop_states"][-1]) <= 1e-6
    bo.close()


# The reference's default driver branch (compile_solver = True: primal warm start, cold
# multipliers; make_golden.py IP_LOOP_CONFIGS), problems of the benchmark batch inside it
IP_LOOPS = [("ip_loop_go2_rnea_n20", "go2", "whole_body_rnea", 20, 64),
            ("ip_loop_b2g_rnea_n50", "b2g", "whole_body_rnea", 50, 1024)]


def test_ip_loop_fixture_first_step_matches_numpy_oracle():
    """The B2G loop fixture comes from the compiled restatement (oracle/cpu); its first solves
    (cold start, the problems shared with the numpy fixture ip_b2g_rnea_n50) agree with the numpy
    oracle's, and the loop holds no failed line search (the benchmark's -2 cascade came from
    carrying lam_g, which the default driver does not do)."""
    L = golden("ip_loop_b2g_rnea_n50.npz")
    G = golden("ip_b2g_rnea_n50.npz")
    shared = 0
    for j, g in enumerate(L["gidx"]):
        for b in range(G["P"].shape[0]):
            if np.array_equal(G["P"][b], L["P"][j]) and np.array_equal(G["X"][b], L["X"][j]):
                assert L["loop_stats"][j, 0].tolist() == [int(G["status"][b]), int(G["iter"][b])]
                assert _rel(L["loop_x"][j, 0], G["x_out"][b]) < 1e-8
                shared += 1
    assert shared >= 3
    # the headline shape's loop never fails a line search; the Go2 loop holds one -2 exit (syn 3,
    # step 4), so the device loop's failure path is pinned too
    assert -2 not in set(L["loop_stats"][:, :, 0].ravel().tolist())
    assert -2 in set(golden("ip_loop_go2_rnea_n20.npz")["loop_stats"][:, :, 0].ravel().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name,rname,dyn,N,B", IP_LOOPS)
def test_ip_gpu_default_driver_loop_inside_batch(name, rname, dyn, N, B):
    """pl_mpc_step with the interior-point solver in the reference's default driver mode (cold
    multipliers per solve, pl_mpc_set_ip_lam(o, 0), the default) over the fixture's steps, inside a
    batch of the benchmark's problems: each fixture problem's status and iteration count exact
    at every step, its iterate x and the state <= 1e-6 relative."""
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    G = golden(f"{name}.npz")
    R = make_robot(rname, "trot")
    lay, P, X, XS, T0 = build_batch(R, dyn, N, B, 0)
    for j, g in enumerate(G["gidx"]):
        assert np.array_equal(P[g], G["P"][j]) and np.array_equal(XS[g], G["XS"][j])
    bo = BatchedOCP(R, dyn, N, batch=B, device=0, gait_type="trot", gait_period=0.8)
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    bo.mpc_setup(XS, T0)
    worst = 0.0
    counts = []
    for k in range(G["loop_states"].shape[1]):
        bo.mpc_step(k)
        st = bo.ip_stats()
        S = bo.mpc_state()
        Xk = bo.get_x()
        counts.append({int(a): int(c) for a, c in zip(*np.unique(st["status"], return_counts=True))})
        for j, g in enumerate(G["gidx"]):
            assert [int(st["status"][g]), int(st["iter"][g])] == G["loop_stats"][j, k].tolist(), (g, k)
            e = max(_rel(S[g], G["loop_states"][j, k]), _rel(Xk[g], G["loop_x"][j, k]))
            worst = max(worst, e)
            assert e <= 1e-6, (g, k, e)
    print(f"{name}: worst {worst:.2e}; status counts per step {counts}")
    bo.close()


@pytest.mark.gpu
def test_ip_gpu_lam_warm_start_matches_oracle():
    """pl_ocp_set_lam: a solve started from given multipliers (the previous solve's lam_g)
    against the oracle's warm start from the same lam0 (stored in the fixture by
    make_golden.py); and set_lam(None) is the cold start."""
    from pinoloco.ocp import BatchedOCP
    G = golden("ip_go2_rnea_n20.npz")
    R = make_robot("go2", "trot")
    B = 2
    bo = BatchedOCP(R, "whole_body_rnea", 20, batch=B, device=0, gait_type="trot")
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"][:B])
    bo.set_x(G["x_out"][:B])
    bo.init_solver()
    bo.set_lam(G["lam"][:B])
    bo.solve()
    X, LAM, st = bo.get_x(), bo.get_lam(), bo.ip_stats()
    for b in range(B):
        assert int(st["status"][b]) == int(G["warm_status"][b]) and int(st["iter"][b]) == int(G["warm_iter"][b]), b
        assert _rel(X[b], G["warm_x"][b]) <= 1e-5 and _rel(LAM[b], G["warm_lam"][b]) <= 1e-5, b
    bo.set_lam(None)  # cold again: the fixture's own solve
    bo.set_x(G["X"][:B])
    bo.solve()
    assert np.array_equal(bo.ip_stats()["iter"], G["iter"][:B].astype(bo.ip_stats()["iter"].dtype))
    assert _rel(bo.get_x()[0], G["x_out"][0]) <= 1e-5
    bo.close()


def _stand_ocp(device):
    """make_ocp(..., solver="fatrop") for the standing fixture, parameters through the
    reference's setters (run_mpc.py:166-176, 127-135)."""
    from pinoloco.ocp import OCP, OCP_ARGS, make_ocp
    R = make_robot("go2", "stand")
    if device >= 0:
        ocp = make_ocp("whole_body_rnea", OCP_ARGS["whole_body_rnea"], robot=R, solver="fatrop", nodes=20)
    else:
        ocp = OCP(R, "fatrop", 20, "whole_body_rnea", device=-1)
        ocp.set_weights()
    ocp.set_time_params(0.01, 0.08)
    ocp.set_swing_params(0.07, [0.1, -0.2])
    ocp.set_tracking_targets(np.zeros(6), np.zeros(3), np.zeros(3))
    ocp.update_initial_state(np.concatenate([R.q0, np.zeros(R.nv)]))
    ocp.update_gait_sequence(0.0)
    ocp.update_previous_torques(np.zeros(R.nj))
    return ocp


def test_make_ocp_setters_reproduce_fixture_params():
    """The setters give the standing fixture's parameter vector bit for bit (host-only)."""
    G = golden("ip_go2_rnea_n20_stand.npz")
    assert np.array_equal(_stand_ocp(-1).param_vector(), G["P"][0])


@pytest.mark.gpu
def test_make_ocp_fatrop_surface():
    """make_ocp(..., solver="fatrop") -> setters -> init_solver -> solve() -> retract / lam_g
    (ocp.py:360-373), at the interior point's trajectory bar (1e-7)."""
    G = golden("ip_go2_rnea_n20_stand.npz")
    ocp = _stand_ocp(0)
    assert np.array_equal(ocp.param_vector(), G["P"][0])
    ocp._x_initial = G["X"][0].copy()  # opti.set_initial: the fixture's standing-equilibrium guess
    ocp.init_solver()
    x = ocp.solve()
    assert ocp.stats["ip_status"] == int(G["status"][0]) and ocp.stats["ip_iter"] == int(G["iter"][0])
    assert _rel(x, G["x_out"][0]) <= TRAJ_TOL
    assert _rel(ocp.lam_g, G["lam"][0]) <= TRAJ_TOL
    assert _rel(ocp.opti.value(ocp.opti.x), G["x_out"][0]) <= TRAJ_TOL
    assert len(ocp.q_sol) == 21


@pytest.mark.gpu
@pytest.mark.parametrize("name,rname,dyn,N,b", [("ip_go2_cv_n20", "go2", "centroidal_vel", 20, 0),
                                                ("ip_go2_cv_n20", "go2", "centroidal_vel", 20, 1),
                                                ("ip_go2_rnea_n20", "go2", "whole_body_rnea", 20, 0),
                                                ("ip_go2_acc_nb_n20", "go2", "whole_body_acc", 20, 1)])
def test_ip_gpu_teacher_forced_directions(name, rname, dyn, N, b):
    """Every iteration's Newton direction from the ORACLE's iterate (teacher forcing, the
    oracle's per-iteration states stored by make_golden.py): dx, dlam, ds <= 1e-8 and the
    fraction-to-boundary steps <= 1e-8 relative, and the same inertia shift.  This pins the
    Lagrangian Hessian, the inertia correction, the linear algebra and the KKT assembly
    independently of the trajectory, which on the infeasible cold starts amplifies 1e-12
    differences through the filter decisions."""
    from pinoloco.ocp import BatchedOCP
    G = golden(f"{name}.npz")
    gait = str(G["gait"])
    R = make_robot(rname, gait)
    ib = bool(int(G["include_base"])) if "include_base" in G else True
    bo = BatchedOCP(R, dyn, N, batch=1, device=0, gait_type=gait, include_base=ib)
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"][b:b + 1])
    bo.init_solver()
    errs = []
    T = {k[len(f"tf{b}_"):]: G[k] for k in G.files if k.startswith(f"tf{b}_")}
    for k in range(T["x"].shape[0]):
        t = {key: v[k] for key, v in T.items()}
        bo.debug_set("ip_dwi", [0.0, float(t["dw_last"])])  # the solve's last inertia shift so far
        dx, dl, ds, am, az = bo.ip_direction(t["x"], t["s"], t["lam"], t["zl"], t["zu"], t["mu"])
        dwi = bo.debug("ip_dwi", 2)[0]
        errs.append(dict(k=k, dx=_rel(dx[0], t["dx"]), dl=_rel(dl[0], t["dl"]), ds=_rel(ds[0], t["ds"]),
                         amax=abs(am[0] - t["amax"]) / max(t["amax"], 1e-300), az=abs(az[0] - t["az"]) / t["az"],
                         dwi=float(dwi), dwi_oracle=float(t["dwi"])))
    os.makedirs(os.path.join(HERE, "..", "gpurun_out"), exist_ok=True)
    with open(os.path.join(HERE, "..", "gpurun_out", f"ip_forced_{name}_{b}.json"), "w") as f:
        json.dump(errs, f, indent=1)
    tol = TF_TOL.get((name, b), 1e-8)
    for e in errs:
        assert max(e["dx"], e["dl"], e["ds"], e["amax"], e["az"]) <= tol, e
        assert e["dwi"] == pytest.approx(e["dwi_oracle"], rel=1e-12, abs=0.0), e
    bo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,rname,dyn,N", IP_FIXTURES)
def test_ip_gpu_lagrangian_hessian(name, rname, dyn, N):
    """k_lag_hess (hyper-dual numbers) against the oracle's complex-step / fourth-order
    difference Hessian of lam^T g at the fixture's solution (OracleOCP.lag_hess, stored by
    make_golden.py): <= 1e-9 relative to max |H| (measured ~1e-11, profiles/r03f)."""
    import scipy.sparse as sp
    from pinoloco.ocp import BatchedOCP
    G = golden(f"{name}.npz")
    gait = str(G["gait"])
    ib = bool(int(G["include_base"])) if "include_base" in G else True
    R = make_robot(rname, gait)
    bo = BatchedOCP(R, dyn, N, batch=1, device=0, gait_type=gait, include_base=ib)
    bo.set_solver("fatrop")
    bo.set_ip_settings()
    bo.set_params(G["P"][:1])
    bo.init_solver()
    bo.ip_direction(G["x_out"][0], G["s"][0], G["lam"][0], G["zl"][0], G["zu"][0], G["mu"][0])
    Hg = bo.lag_hess()[0]
    bo.close()
    Ho = sp.csr_matrix((G["hess_data"], G["hess_indices"], G["hess_indptr"]), shape=Hg.shape)
    assert abs(Hg - Ho).max() <= 1e-9 * abs(Ho).max()


@pytest.mark.gpu
def test_ip_gpu_gauss_newton_option():
    """pl_ip_settings.hessian = PL_IP_HESS_GN: the objective's diagonal only (no Lagrangian
    curvature, no inertia correction), against the oracle with hessian="gauss_newton"."""
    from oracle.ip_ref import IPRef
    from oracle.ocp import OracleOCP
    from pinoloco.ocp import BatchedOCP
    G = golden("ip_go2_rnea_n20_stand.npz")
    R = make_robot("go2", "stand")
    bo = BatchedOCP(R, "whole_body_rnea", 20, batch=1, device=0, gait_type="stand")
    bo.set_solver("fatrop")
    bo.set_ip_settings(hessian="gauss_newton")
    bo.set_params(G["P"][:1])
    bo.set_x(G["X"][:1])
    bo.init_solver()
    bo.solve()
    x, lam, so = IPRef(OracleOCP(R, "whole_body_rnea", 20), {"hessian": "gauss_newton"}).solve(G["X"][0], G["P"][0])
    st = bo.ip_stats()
    assert int(st["status"][0]) == so["status"] and int(st["iter"][0]) == so["iter"]
    assert _rel(bo.get_x()[0], x) <= 1e-5 and _rel(bo.get_lam()[0], lam) <= 1e-5
    bo.close()


def _run_mpc_setup(device):
    """run_mpc.py:13-37 and main() (:147-176): B2G standing_with_arm_up, whole_body_rnea,
    nodes 14, trot 0.8, dt 0.01 / 0.08, the tracking targets and swing parameters."""
    from pinoloco.ocp import OCP, OCP_ARGS, make_ocp
    from pinoloco.robots import B2G
    robot = B2G(reference_pose="standing_with_arm_up", ignore_arm=False)
    robot.set_gait_sequence("trot", 0.8)
    if device >= 0:
        ocp = make_ocp(dynamics="whole_body_rnea", default_args=OCP_ARGS["whole_body_rnea"], robot=robot, nodes=14,
                       solver="fatrop")
    else:  # host-only handle (no GPU): the same OCP class surface
        ocp = OCP(robot, "fatrop", 14, "whole_body_rnea", device=-1)
        ocp.set_weights()
    ocp.set_time_params(0.01, 0.08)
    ocp.set_swing_params(0.07, [0.1, -0.2])
    ocp.set_tracking_targets(np.array([0.2, 0, 0, 0, 0, 0]), np.array([0, 0, 0]), np.array([0, 0, 0]))
    return robot, ocp


def _compiled_params(ocp, robot, x_init, k, Q_diag, R_diag, W_diag, tau_prev, warm_start=True):
    """One iteration's parameter list, as run_mpc.py:70-96 builds it."""
    dt_min, dt_max = 0.01, 0.08
    t_current = k * dt_min
    ocp.update_initial_state(x_init)
    ocp.update_gait_sequence(t_current)
    contact_schedule = ocp.opti.value(ocp.contact_schedule)
    swing_schedule = ocp.opti.value(ocp.swing_schedule)
    n_contacts = ocp.opti.value(ocp.n_contacts)
    swing_period = ocp.opti.value(ocp.swing_period)
    params = [x_init, dt_min, dt_max, contact_schedule, swing_schedule, n_contacts,
              swing_period, 0.07, [0.1, -0.2], Q_diag, R_diag, np.array([0.2, 0, 0, 0, 0, 0])]
    if ocp.ext_force_frame:
        params += [np.array([0, 0, 0])]
    if ocp.arm_ee_frame:
        params += [np.array([0, 0, 0])]
    if warm_start:
        ocp.warm_start()
        x_warm_start = ocp.opti.value(ocp.opti.x, ocp.opti.initial())
        params += [x_warm_start]
    params += [tau_prev, W_diag]
    return params


def test_compiled_solver_surface():
    """compile_solver / solver_function / opti.value (ocp.py:324-342, ocp_whole_body_rnea.py:
    237-258, run_mpc.py:56-100) on a host-only handle: the argument list of the reference's
    generated function, its packing into the parameter vector (bit-equal to the setters'
    and to the oracle loop's first step, tests/golden/ip_b2g_rnea_n14_compiled.npz), and
    the arity check."""
    from pinoloco.ocp import OCP
    robot, ocp = _run_mpc_setup(-1)
    ocp.update_initial_state(ocp.x_nom)
    ocp.update_gait_sequence(0.0)
    ocp.compile_solver(True)
    f = ocp.solver_function
    assert f.n_in() == 17 and f.names[12:] == ["ext_force_des", "arm_vel_des", "x", "tau_prev", "W_diag"]
    Q, R, W = ocp.opti.value(ocp.Q_diag), ocp.opti.value(ocp.R_diag), ocp.opti.value(ocp.W_diag)
    params = _compiled_params(ocp, robot, ocp.x_nom, 0, Q, R, W, np.zeros(robot.nj))
    p, x0 = f._pack(params)
    assert np.array_equal(p, ocp.param_vector())
    G = golden("ip_b2g_rnea_n14_compiled.npz")
    assert np.array_equal(p, G["P"][0]) and np.array_equal(x0, G["X0"][0])
    with pytest.raises(TypeError):
        f(*params[:-1])
    ocp.compile_solver(False)  # without the warm start the initial guess is baked in
    assert ocp.solver_function.n_in() == 16 and "x" not in ocp.solver_function.names
    go2 = OCP(make_robot("go2"), "fatrop", 20, "whole_body_rnea", device=-1)
    go2.compile_solver(True)
    assert go2.solver_function.n_in() == 15  # no ext force / arm targets
    osqp = OCP(make_robot("go2"), "osqp", 20, "whole_body_rnea", device=-1)
    osqp.compile_solver(True)
    assert osqp.solver_function is None
    assert ocp.opti.value(0.25) == 0.25  # plain numbers (the dts) pass through


@pytest.mark.gpu
def test_run_mpc_compiled_fatrop_branch():
    """The reference's default driver configuration -- solver "fatrop", compile_solver = True,
    warm_start = True (run_mpc.py:34-37) -- through mpc_loop's compiled branch (run_mpc.py:
    50-113) verbatim for 3 steps, against the oracle's loop (make_golden.py
    ip_compiled_fixture): per step the interior point's status and iteration count exact, sol_x <= 1e-7 and the next x_init
    <= 1e-7 relative (the first step's parameters and warm start bit-equal, later ones <= 1e-7:
    they carry the previous solves' round-off)."""
    robot, ocp = _run_mpc_setup(0)
    G = golden("ip_b2g_rnea_n14_compiled.npz")
    warm_start = True
    x_init = ocp.x_nom
    tau_prev = np.zeros(robot.nj)
    ocp.init_solver()
    ocp.compile_solver(warm_start)
    solver_function = ocp.solver_function
    Q_diag = ocp.opti.value(ocp.Q_diag)
    R_diag = ocp.opti.value(ocp.R_diag)
    W_diag = ocp.opti.value(ocp.W_diag)
    errs = []
    for k in range(G["P"].shape[0]):
        params = _compiled_params(ocp, robot, x_init, k, Q_diag, R_diag, W_diag, tau_prev, warm_start)
        p, x0 = solver_function._pack(params)
        if k == 0:  # from x_nom: the same parameters bit for bit
            assert np.array_equal(p, G["P"][k]) and np.array_equal(x0, G["X0"][k])
        else:  # x_init, tau_prev and the warm start carry the previous solves' round-off
            assert _rel(p, G["P"][k]) <= 1e-7 and _rel(x0, G["X0"][k]) <= 1e-7, k
        sol_x = solver_function(*params)
        st = ocp.stats
        assert (int(st["ip_status"]), int(st["ip_iter"])) == (int(G["status"][k]), int(G["iter"][k])), (k, st)
        ocp.retract_stacked_sol(sol_x, retract_all=False)
        x_init = ocp.dyn.state_integrate()(x_init, ocp.DX_prev[1])
        tau_prev = ocp.get_tau_sol(i=1)
        errs.append((_rel(sol_x, G["x_out"][k]), _rel(x_init, G["x_init_next"][k])))
        assert errs[-1][0] <= 1e-7 and errs[-1][1] <= 1e-7, (k, errs)
    ocp._backend.close()


@pytest.mark.gpu
def test_run_mpc_load_compiled_solver_external():
    """The reference's hardware-deployment path: load_compiled_solver (run_mpc.py:51-53),
    solver_function = ca.external("compiled_solver", lib), here the library's own
    compiled_solver symbol in CasADi's external ABI (include/pinoloco_casadi.h), driven through
    casadi_ext.ExternalFunction exactly as CasADi calls it (n_in / sparsity / work / call).
    The loop of run_mpc.py:68-111 for 3 steps against the oracle's loop
    (ip_b2g_rnea_n14_compiled.npz): status / iterations exact, sol_x and the next x_init <= 1e-7."""
    from pinoloco import casadi_ext
    robot, ocp = _run_mpc_setup(0)
    G = golden("ip_b2g_rnea_n14_compiled.npz")
    warm_start = True
    x_init = ocp.x_nom
    tau_prev = np.zeros(robot.nj)
    ocp.init_solver()
    casadi_ext.bind_compiled(ocp, warm_start)
    solver_function = casadi_ext.ExternalFunction("compiled_solver")
    assert solver_function.n_in == 17 and solver_function.n_out == 1
    Q_diag = ocp.opti.value(ocp.Q_diag)
    R_diag = ocp.opti.value(ocp.R_diag)
    W_diag = ocp.opti.value(ocp.W_diag)
    for k in range(G["P"].shape[0]):
        params = _compiled_params(ocp, robot, x_init, k, Q_diag, R_diag, W_diag, tau_prev, warm_start)
        (sol_x,) = solver_function(*params)
        sol_x = np.asarray(sol_x).ravel()
        st = ocp._backend.ip_stats()
        assert (int(st["status"][0]), int(st["iter"][0])) == (int(G["status"][k]), int(G["iter"][k])), k
        ocp.retract_stacked_sol(sol_x, retract_all=False)
        x_init = ocp.dyn.state_integrate()(x_init, ocp.DX_prev[1])
        tau_prev = ocp.get_tau_sol(i=1)
        assert _rel(sol_x, G["x_out"][k]) <= 1e-7 and _rel(x_init, G["x_init_next"][k]) <= 1e-7, k
    with pytest.raises(ValueError):
        solver_function(*params[:-1])
    casadi_ext.unbind()
    ocp._backend.close()


def test_compiled_solver_symbols_host_only():
    """compiled_solver's CasADi symbols on a host-only handle: binding refuses a handle that is
    not an interior-point batch-1 OCP, and the export set includes the compiled solver."""
    from pinoloco import _lib, casadi_ext
    from pinoloco.ocp import BatchedOCP
    L = _lib.lib()
    for suffix in ("", "_n_in", "_n_out", "_sparsity_in", "_sparsity_out", "_work", "_name_in"):
        assert hasattr(L, "compiled_solver" + suffix)
    bo = BatchedOCP(make_robot("go2"), "whole_body_rnea", 20, batch=2, device=-1)
    with pytest.raises(_lib.PinolocoError):
        casadi_ext.bind_compiled(bo, True)  # osqp solver, batch 2
    bo.close()
    assert "compiled_solver" in casadi_ext.FUNCTIONS
