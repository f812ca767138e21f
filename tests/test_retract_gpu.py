"""Batched device-side retract (pl_ocp_retract / pl_ocp_retract_device, k_retract.hip) on the
MI355X: q, v, a, forces, tau and eom_base of every (problem, node) against the oracle, composed
as tests/test_casadi_ext.py composes the host export's check (the same node code, retract.h,
produces both), with that file's bars for the same quantity and variant:

* q / v: 1e-12 absolute; inputs copied through (forces, the a / tau blocks of u) bit-equal;
* whole_body_aba a = ABA: 1e-10 relative to max(1, |.|); the same bar for the base acceleration
  solved from the base equations without the base (tests/test_dynamics.py's bar for
  base_acc_dynamics);
* RNEA tau: 1e-12 relative to max(1, |.|); eom_base, rows 0:6 of the same RNEA call, the same
  bar relative to max(1, max |RNEA output|).  Where a is itself solved on the device (ABA, the
  base solve) the oracle's RNEA is evaluated at the device's a, which has its own bar above: the
  RNEA bar then measures the RNEA call, not the acceleration error times the inertia;
* centroidal_vel: q 1e-13, v 1e-11, a and tau (hence eom_base) 1e-9 relative, the bars of
  test_retract_solution_centroidal_vel_without_base.

Shapes: N = 6 with tau_nodes = 3 (both tau rules of whole_body_rnea), batch 3, steps in {2, N}."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime; the device buffers below)

from conftest import golden, make_robot

pytestmark = pytest.mark.gpu

N, B = 6, 3
FIELDS = ("q", "v", "a", "forces", "tau", "eom_base")
VARIANTS = [("go2", "whole_body_rnea", {}),
            ("go2", "whole_body_rnea", {"include_acc": False}),
            ("go2", "whole_body_acc", {}),
            ("go2", "whole_body_acc", {"include_base": False}),
            ("go2", "whole_body_aba", {}),
            ("go2", "centroidal_vel", {}),
            ("go2", "centroidal_vel", {"include_base": False}),
            ("go2", "centroidal_acc", {}),
            ("go2", "centroidal_acc", {"include_base": False}),
            ("b2g", "whole_body_rnea", {})]
IDS = [f"{r}-{d}" + "".join(f"-{k}0" for k in kw) for r, d, kw in VARIANTS]
SENTINEL = -1.2345e300
PAD = 64

_cache = {}


def _inputs(rname, dyn, kw):
    """P (distinct x_init per problem: synthetic problems 0..B-1) and X = seeded normal x 0.1."""
    from pinoloco.synthetic import build_batch
    R = make_robot(rname)
    lay, P, _, _, _ = build_batch(R, dyn, N, B, 0, **kw)
    assert not np.array_equal(P[0, :lay.nx], P[1, :lay.nx])
    X = np.random.default_rng(3).normal(size=(B, lay.n)) * 0.1
    return R, lay, P, X


def _case(k):
    """One device run per variant (batch 3, every node, the terminal row), shared by the tests."""
    if k not in _cache:
        from pinoloco.ocp import BatchedOCP
        rname, dyn, kw = VARIANTS[k]
        R, lay, P, X = _inputs(rname, dyn, kw)
        bo = BatchedOCP(R, dyn, N, batch=B, device=0, **kw)
        bo.set_params(P)
        bo.set_x(X)
        full = bo.retract(N, True)
        _cache[k] = (R, lay, P, X, bo, full)
    return _cache[k]


def _relmax(got, want, scale=None):
    s = max(1.0, np.abs(want if scale is None else scale).max()) if np.size(want) else 1.0
    return (np.abs(got - want).max() / s) if np.size(want) else 0.0


def _check_problem(R, dyn, kw, lay, p, x, got):
    """Every row of one problem against the oracle; prints each error figure before asserting."""
    from oracle import rbd
    from oracle.ocp import OracleOCP
    from pinoloco.gait import horizon_dts
    from pinoloco.synthetic import DT_MAX, DT_MIN
    o = OracleOCP(R, dyn, N, **kw)
    M = rbd.ModelArrays(R.model)
    frames = list(R.foot_frames) + ([R.ext_force_frame] if R.ext_force_frame is not None else [])
    nq, nv, nj, nf = R.nq, R.nv, R.nj, R.nf
    x_init = p[lay.poff["x_init"][0]:lay.poff["x_init"][0] + lay.nx]
    dts = horizon_dts(DT_MIN, DT_MAX, N)
    DX, U = o.split(x)
    cv = dyn == "centroidal_vel"
    base = kw.get("include_base", True)
    fd = dyn == "whole_body_rnea" and not kw.get("include_acc", True)
    assert got["tau"].shape == (N, nj) and got["eom_base"].shape == (N, 6) and got["forces"].shape == (N, nf)
    assert got["a"].shape == (N, 0 if fd else nv)
    assert got["q"].shape == (N + 1, nq) and got["v"].shape == (N if cv else N + 1, nv)
    worst = {}

    def bar(name, err, tol):
        worst[name] = max(worst.get(name, 0.0), err)
        assert err < tol, (name, err, tol)

    for i in range(N):
        xs = o.integrate_state(x_init, DX[i])
        u = U[i]
        if cv:
            h, qi = xs[:6], xs[6:]
            nvo = nv if base else nj

            def vel(uu):  # both velocities of a difference at this node's h, q (ocp_centroidal_vel.py:240-246)
                return uu[:nvo] if base else np.concatenate([rbd.base_vel_cv(M, h, qi, uu[:nvo], R.mass), uu[:nvo]])
            vi, f = vel(u), u[nvo:]
            k = i if i + 1 < N else i - 1  # the last node reuses the previous node's difference
            a_j = ((vel(U[k + 1]) - vel(U[k])) / dts[k])[6:]
            want_a = np.concatenate([rbd.base_acc_cv(M, frames, qi, vi, a_j, f, R.mass), a_j])
            rn = rbd.rnea_dynamics(M, frames, qi, vi, want_a, f)
            bar("q", np.abs(got["q"][i] - qi).max(), 1e-13)
            if base:
                assert np.array_equal(got["v"][i], vi), i
            else:
                bar("v", _relmax(got["v"][i], vi), 1e-11)
            bar("a", _relmax(got["a"][i], want_a), 1e-9)
            assert np.array_equal(got["forces"][i], f), i
            bar("tau", _relmax(got["tau"][i], rn[6:]), 1e-9)
            bar("eom_base", _relmax(got["eom_base"][i], rn[:6], rn), 1e-9)
            continue
        qi, vi = xs[:nq], xs[nq:]
        bar("q", np.abs(got["q"][i] - qi).max(), 1e-12)
        bar("v", np.abs(got["v"][i] - vi).max(), 1e-12)
        if dyn == "whole_body_aba":
            tau_j, f = u[:nj], u[nj:]
            want_a = rbd.aba_dynamics(M, frames, qi, vi, tau_j, f)
            bar("a", _relmax(got["a"][i], want_a), 1e-10)
            assert np.array_equal(got["tau"][i], tau_j), i
            a_rn = got["a"][i]
        elif dyn in ("whole_body_acc", "centroidal_acc") and not base:
            a_j, f = u[:nj], u[nj:]
            want_a = np.concatenate([rbd.base_acc_wb(M, frames, qi, vi, a_j, f), a_j])
            bar("a", _relmax(got["a"][i], want_a), 1e-10)
            assert np.array_equal(got["a"][i][6:], a_j), i
            a_rn = got["a"][i]
        elif fd:  # a = (v_{i+1} - v_i) / dt_i, not an output (ocp_whole_body_rnea.py:183-191)
            f = u[:nf]
            a_rn = (o.integrate_state(x_init, DX[i + 1])[nq:] - vi) / dts[i]
        else:
            a_rn, f = u[:nv], u[nv:nv + nf]
            assert np.array_equal(got["a"][i], a_rn), i
        assert np.array_equal(got["forces"][i], f), i
        rn = rbd.rnea_dynamics(M, frames, qi, vi, a_rn, f)
        if dyn == "whole_body_rnea" and i < lay.tau_nodes:
            assert np.array_equal(got["tau"][i], u[lay.na + nf:]), i
        elif dyn != "whole_body_aba":  # nodes without a tau variable: the RNEA joint rows
            bar("tau", _relmax(got["tau"][i], rn[6:]), 1e-12)
        bar("eom_base", _relmax(got["eom_base"][i], rn[:6], rn), 1e-12)
    xs = o.integrate_state(x_init, DX[N])
    if cv:
        bar("q", np.abs(got["q"][N] - xs[6:]).max(), 1e-13)
    else:
        bar("q", np.abs(got["q"][N] - xs[:nq]).max(), 1e-12)
        bar("v", np.abs(got["v"][N] - xs[nq:]).max(), 1e-12)
    print("retract errors", dyn, kw, {k: f"{v:.2e}" for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("k", range(len(VARIANTS)), ids=IDS)
def test_retract_matches_oracle(k):
    """Every row of every problem, each with its own x_init.  Covers by value: centroidal_vel's
    node N - 1 (the previous node's difference, pinoloco/ocp.py OCPCentroidalVel), whole_body_rnea
    nodes 3..5 (tau from RNEA) and include_acc=False (a has no columns; tau and eom_base from the
    finite-difference a)."""
    R, lay, P, X, bo, full = _case(k)
    rname, dyn, kw = VARIANTS[k]
    for b in range(B):
        worst = _check_problem(R, dyn, kw, lay, P[b], X[b], {f: full[f][b] for f in FIELDS})
        if dyn == "whole_body_rnea":
            assert "tau" in worst  # a node past tau_nodes was compared with RNEA
    assert all(np.all(np.isfinite(full[f])) for f in FIELDS)


@pytest.mark.parametrize("k", range(len(VARIANTS)), ids=IDS)
def test_batch_and_steps_invariance(k):
    """Problem b of the batch equals a batch-1 handle with the same P[b], X[b], and the rows of
    steps=2 equal rows 0-1 of steps=N, bit for bit."""
    from pinoloco.ocp import BatchedOCP
    R, lay, P, X, bo, full = _case(k)
    rname, dyn, kw = VARIANTS[k]
    short = bo.retract(2, False)
    plain = bo.retract(N, False)
    for f in FIELDS:
        assert short[f].shape[1] == 2 and plain[f].shape[1] == N
        assert np.array_equal(short[f], full[f][:, :2]), f
        assert np.array_equal(plain[f], full[f][:, :N]), f
    for b in range(B):
        b1 = BatchedOCP(R, dyn, N, batch=1, device=0, **kw)
        b1.set_params(P[b:b + 1])
        b1.set_x(X[b:b + 1])
        one = b1.retract(N, True)
        b1.close()
        for f in FIELDS:
            assert np.array_equal(one[f][0], full[f][b]), (b, f)


@pytest.mark.parametrize("k", [0, 1, 5, 9], ids=[IDS[j] for j in (0, 1, 5, 9)])
@pytest.mark.parametrize("steps,terminal", [(2, False), (N, True)])
def test_no_writes_outside_the_result(k, steps, terminal):
    """Host arrays and the device destination carry 64 sentinel doubles at each end that must
    survive; the device variant equals the host variant bit for bit."""
    from pinoloco import _lib
    R, lay, P, X, bo, full = _case(k)
    sz = bo.retract_sizes(steps, terminal)
    host = {}
    for f in FIELDS:
        host[f] = np.full(2 * PAD + B * sz[f]["rows"] * sz[f]["width"], SENTINEL)
    ptrs = [host[f][PAD:].ctypes.data_as(C.POINTER(C.c_double)) for f in FIELDS]
    _lib.check(_lib.lib().pl_ocp_retract(bo.h, steps, int(terminal), *ptrs))
    dev = torch.full((sz["total"] + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    bo.retract_device(dev.data_ptr() + 8 * PAD, steps, terminal)
    packed = dev.cpu().numpy()
    assert np.all(packed[:PAD] == SENTINEL) and np.all(packed[-PAD:] == SENTINEL)
    body = packed[PAD:-PAD]
    assert not np.any(body == SENTINEL)  # and every double of the result was written
    for f in FIELDS:
        n = B * sz[f]["rows"] * sz[f]["width"]
        assert np.all(host[f][:PAD] == SENTINEL) and np.all(host[f][PAD + n:] == SENTINEL), f
        got = host[f][PAD:PAD + n].reshape(B, sz[f]["rows"], sz[f]["width"])
        assert np.array_equal(got, full[f][:, :sz[f]["rows"]]), f
        assert np.array_equal(body[sz[f]["offset"]:sz[f]["offset"] + n], got.ravel()), f
    # fields passed as NULL are skipped, the others unchanged
    q = np.zeros((B, sz["q"]["rows"], sz["q"]["width"]))
    _lib.check(_lib.lib().pl_ocp_retract(bo.h, steps, int(terminal), _lib.dptr(q), None, None, None, None, None))
    assert np.array_equal(q, full["q"][:, :sz["q"]["rows"]])


def test_drop_in_solve_retract_matches_the_backend():
    """make_ocp("whole_body_aba").solve(retract_all=True) (the host loop retract_stacked_sol,
    ocp_whole_body_aba.py:177-214) and the backend's device retract of the same solution."""
    from pinoloco.ocp import OCP_ARGS, make_ocp
    from pinoloco.synthetic import DT_MAX, DT_MIN, SWING_HEIGHT, SWING_VEL_LIMITS, random_state
    R = make_robot("go2")
    Nn = 12
    xs, t0, vx = random_state(R, 3)
    ocp = make_ocp("whole_body_aba", OCP_ARGS["whole_body_aba"], robot=R, nodes=Nn, solver="osqp")
    ocp.set_time_params(DT_MIN, DT_MAX)
    ocp.set_swing_params(SWING_HEIGHT, list(SWING_VEL_LIMITS))
    ocp.set_tracking_targets([vx, 0, 0, 0, 0, 0], [0, 0, 0], [0, 0, 0])
    ocp.update_initial_state(xs)
    ocp.update_gait_sequence(t0)
    ocp.init_solver()
    ocp.solve(retract_all=True)
    got = ocp._backend.retract(steps=Nn, terminal=True)
    assert len(ocp.q_sol) == Nn + 1 and len(ocp.a_sol) == Nn
    for i in range(Nn + 1):
        assert np.abs(got["q"][0, i] - ocp.q_sol[i]).max() < 1e-12, i
        assert np.abs(got["v"][0, i] - ocp.v_sol[i]).max() < 1e-12, i
    for i in range(Nn):
        want_a = np.asarray(ocp.a_sol[i]).ravel()
        assert np.abs(got["a"][0, i] - want_a).max() < 1e-10 * max(1.0, np.abs(want_a).max()), i
        assert np.array_equal(got["forces"][0, i], ocp.forces_sol[i]), i
        assert np.array_equal(got["tau"][0, i], ocp.tau_sol[i]), i


def test_retract_inside_the_mpc_loop():
    """After each pl_mpc_step the parameters hold that step's x_init and the iterate its
    solution: node 1 of the retract is the next state, integrate(x_init, DX[1]) (run_mpc.py:142),
    which k_mpc_finish computed with the same integrate (1e-13: contraction may differ between the
    two kernels).  Retract calls between the steps leave the captured graph alone."""
    from pinoloco.ocp import BatchedOCP
    G = golden("sqp_go2_rnea_n20.npz")
    R = make_robot("go2")
    Bm = 4
    bo = BatchedOCP(R, "whole_body_rnea", 20, batch=Bm, device=0)
    bo.set_params(G["P"][:Bm])
    bo.set_x(G["X"][:Bm])
    bo.init_solver()
    bo.mpc_setup(G["XS"][:Bm], G["T0"][:Bm])
    infos = []
    for k in range(3):
        bo.mpc_step(k)
        got = bo.retract(steps=3)
        xs = bo.mpc_state()
        err = max(np.abs(got["q"][:, 1] - xs[:, :R.nq]).max(), np.abs(got["v"][:, 1] - xs[:, R.nq:]).max())
        print("mpc step", k, "node-1 state error", err)
        assert err < 1e-13, (k, err)
        infos.append(bo.mpc_graph_info())
    assert [i["captures"] for i in infos] == [0, 1, 1], infos
    assert all(i["eager_fallback"] == 0 for i in infos), infos
    assert infos[-1]["replays"] == 2, infos
    bo.close()


def teardown_module(module):
    for case in _cache.values():
        case[4].close()
    _cache.clear()
