"""The plant of the device MPC loop (pl_mpc_set_plant / pl_mpc_set_disturbance, k_plant.hip,
plant.h) on the MI355X.

With PL_PLANT_ABA the true state x_state is stepped, after every solve, through the forward
dynamics under node 0's commanded torques and forces and a base wrench.  The numpy plant below
is the same composition from the oracle's own pieces: rbd.aba with the base rows of tau set to
the wrench, rbd.contact_fext for the world-aligned forces, rbd.integrate for the state map.  It
is applied to mpc_state() before the step, with the tau and forces that the device's retract
of node 0 returns after the step (the retract has its own tests, tests/test_retract_gpu.py, so
the bar here measures the plant).

Bars: the state after the step against the numpy plant at the project's ABA bar
(tests/test_retract_gpu.py), 1e-10 x max(1, max |a| over the problem's substeps), used for the
state itself: every substep scales the acceleration error by h <= 0.012, so the bar is loose by
construction.  x_init under state noise at the q / v bar of the retract tests, 1e-12.

Shapes: the retract tests': N = 6 with tau_nodes = 3, batch 3, synthetic problems, three MPC
steps.  Each problem has its own dt_min (the plant's h is the problem's own parameter)."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime)

from conftest import make_robot

pytestmark = pytest.mark.gpu

N, B, STEPS = 6, 3, 3
VARIANTS = [("go2", "whole_body_rnea", {}),
            ("go2", "whole_body_rnea", {"include_acc": False}),
            ("go2", "whole_body_acc", {}),
            ("go2", "whole_body_acc", {"include_base": False}),
            ("go2", "whole_body_aba", {}),
            ("go2", "centroidal_acc", {}),
            ("go2", "centroidal_acc", {"include_base": False}),
            ("b2g", "whole_body_rnea", {})]
IDS = [f"{r}-{d}" + "".join(f"-{k}0" for k in kw) for r, d, kw in VARIANTS]
ABA_BAR = 1e-10
QV_BAR = 1e-12


def _wrench(batch, seed=5):
    """A distinct non-zero base wrench per problem: tens of newtons, a few newton metres."""
    return np.random.default_rng(seed).normal(size=(batch, 6)) * np.array([20.0, 20.0, 20.0, 3.0, 3.0, 3.0])


def _start(rname, dyn, kw, nodes=N, batch=B, debug_paths=(), solver=None):
    """A handle ready for mpc_step(0) on synthetic problems 0..batch-1, each with its own dt_min."""
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import DT_MIN, build_batch
    R = make_robot(rname)
    lay, P, X, XS, T0 = build_batch(R, dyn, nodes, batch, 0, **kw)
    P = P.copy()
    P[:, lay.poff["dt_min"][0]] = DT_MIN * (1.0 + 0.1 * np.arange(batch))
    bo = BatchedOCP(R, dyn, nodes, batch=batch, device=0, debug_paths=debug_paths, **kw)
    if solver is not None:
        bo.set_solver(solver)
        bo.set_ip_settings()
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    bo.mpc_setup(XS, T0)
    return R, lay, P, bo


def _frames(R):
    return list(R.foot_frames) + ([R.ext_force_frame] if R.ext_force_frame is not None else [])


def _numpy_plant(M, frames, nq, xs, tau, f, w, dt_min, substeps):
    """substeps x { a = ABA(q, v, [w; tau], f); q <- integrate(q, v h); v <- v + a h }; also max |a|."""
    from oracle import rbd
    q, v = xs[:nq].copy(), xs[nq:].copy()
    h = dt_min / substeps
    amax = 0.0
    for _ in range(substeps):
        _, oM = rbd.forward_kinematics(M, q)
        a = rbd.aba(M, q, v, np.concatenate([w, tau]), rbd.contact_fext(M, oM, frames, f))
        amax = max(amax, np.abs(a).max())
        q = rbd.integrate(M, q, v * h)
        v = v + a * h
    return np.concatenate([q, v]), amax


def _check_step(R, M, lay, P, before, after, ret, W, substeps, worst):
    """Every problem's state after one step against the numpy plant; the figures into `worst`."""
    nq = R.nq
    fails = []
    for b in range(before.shape[0]):
        want, amax = _numpy_plant(M, _frames(R), nq, before[b], ret["tau"][b, 0], ret["forces"][b, 0], W[b],
                                  P[b, lay.poff["dt_min"][0]], substeps)
        tol = ABA_BAR * max(1.0, amax)
        eq, ev = np.abs(after[b, :nq] - want[:nq]).max(), np.abs(after[b, nq:] - want[nq:]).max()
        worst["q"], worst["v"] = max(worst.get("q", 0.0), eq), max(worst.get("v", 0.0), ev)
        worst["amax"] = max(worst.get("amax", 0.0), amax)
        if not (eq < tol and ev < tol):
            fails.append((b, eq, ev, tol))
    return fails


def _run_plant(bo, R, lay, P, W, substeps, steps=STEPS, tag=""):
    from oracle import rbd
    M = rbd.ModelArrays(R.model)
    worst, fails, states = {}, [], []
    for k in range(steps):
        before = bo.mpc_state()
        bo.mpc_step(k)
        ret = bo.retract(1)
        after = bo.mpc_state()
        assert np.all(np.isfinite(after)), k
        assert not np.array_equal(after, before), k
        fails += [(k,) + f for f in _check_step(R, M, lay, P, before, after, ret, W, substeps, worst)]
        states.append(after)
    print("plant errors", tag, f"substeps={substeps}", {k: f"{v:.2e}" for k, v in worst.items()})
    assert not fails, fails
    return states


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("k", range(len(VARIANTS)), ids=IDS)
def test_plant_matches_numpy(k, substeps):
    """Three closed-loop steps under a distinct non-zero wrench per problem: tau from u (rnea,
    aba) or from the RNEA joint rows (acc, centroidal_acc), the base solved or not, the
    finite-difference rnea, and B2G's external-force frame (nf = 15)."""
    rname, dyn, kw = VARIANTS[k]
    R, lay, P, bo = _start(rname, dyn, kw)
    W = _wrench(B)
    bo.mpc_set_plant("aba", substeps)
    bo.mpc_set_disturbance(base_wrench=W)
    try:
        _run_plant(bo, R, lay, P, W, substeps, tag=IDS[k])
    finally:
        bo.close()


def _loop(bo, steps):
    states = []
    for k in range(steps):
        bo.mpc_step(k)
        states.append(bo.mpc_state())
    return states


def test_default_loop_untouched():
    """mpc_set_plant("nominal") and cleared disturbances are the loop of a handle that never
    called the new interface, bit for bit."""
    _, _, _, plain = _start("go2", "whole_body_rnea", {})
    _, _, _, named = _start("go2", "whole_body_rnea", {})
    named.mpc_set_plant("nominal")
    named.mpc_set_disturbance()
    a, b = _loop(plain, STEPS), _loop(named, STEPS)
    for k in range(STEPS):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(plain.get_x(), named.get_x())
    assert np.array_equal(plain.get_params(), named.get_params())
    plain.close()
    named.close()


def test_problems_are_independent():
    """A wrench on problem 1 alone moves problem 1 alone."""
    _, _, _, calm = _start("go2", "whole_body_rnea", {})
    _, _, _, pushed = _start("go2", "whole_body_rnea", {})
    W = np.zeros((B, 6))
    W[1] = _wrench(B)[1]
    for bo in (calm, pushed):
        bo.mpc_set_plant("aba", 2)
    pushed.mpc_set_disturbance(base_wrench=W)
    a, b = _loop(calm, STEPS), _loop(pushed, STEPS)
    for k in range(STEPS):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][2], b[k][2]), k
        assert not np.array_equal(a[k][1], b[k][1]), k
    xa, xb = calm.get_x(), pushed.get_x()
    assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[2], xb[2]) and not np.array_equal(xa[1], xb[1])
    calm.close()
    pushed.close()


def _noise(lay, seed=9):
    """Rows 0 and 2 drawn (millimetres / milliradians, cm/s), row 1 zero with the flag on."""
    z = np.random.default_rng(seed).normal(size=(B, lay.ndx)) * 1e-2
    z[1] = 0.0
    return z


def _integrate_state(M, R, dyn, xs, dz):
    from oracle import rbd
    if dyn == "centroidal_vel":  # x = [h, q]
        return np.concatenate([xs[:6] + dz[:6], rbd.integrate(M, xs[6:], dz[6:])])
    return np.concatenate([rbd.integrate(M, xs[:R.nq], dz[:R.nv]), xs[R.nq:] + dz[R.nv:]])


def test_state_noise_with_the_aba_plant():
    """The MPC plans from x_init = state_integrate(x_state, noise); the plant still steps the true
    state, under the torques planned from the measured one."""
    from oracle import rbd
    R, lay, P, bo = _start("go2", "whole_body_rnea", {})
    M = rbd.ModelArrays(R.model)
    W, Z = _wrench(B), _noise(lay)
    bo.mpc_set_plant("aba", 2)
    bo.mpc_set_disturbance(base_wrench=W, state_noise=Z)
    o, worst, fails, werr = lay.poff["x_init"][0], {}, [], 0.0
    for k in range(STEPS):
        before = bo.mpc_state()
        bo.mpc_step(k)
        xi = bo.get_params()[:, o:o + lay.nx]
        after = bo.mpc_state()
        for b in range(B):
            err = np.abs(xi[b] - _integrate_state(M, R, "whole_body_rnea", before[b], Z[b])).max()
            werr = max(werr, err)
            assert err < QV_BAR, (k, b, err)
            if np.any(Z[b]):
                assert not np.array_equal(xi[b], before[b]), (k, b)
        fails += [(k,) + f for f in _check_step(R, M, lay, P, before, after, bo.retract(1), W, 2, worst)]
    print("noise: x_init error", f"{werr:.2e}", "plant errors", {k: f"{v:.2e}" for k, v in worst.items()})
    assert not fails, fails
    # switched off again: the plain copy, bit for bit
    bo.mpc_set_disturbance(base_wrench=W)
    before = bo.mpc_state()
    bo.mpc_step(STEPS)
    assert np.array_equal(bo.get_params()[:, o:o + lay.nx], before)
    bo.close()


@pytest.mark.parametrize("dyn", ["whole_body_rnea", "centroidal_vel"])
def test_state_noise_with_the_nominal_plant(dyn):
    """The noise applies under the default plant too, and to centroidal_vel's x = [h, q]:
    x_init is the measured state, x_state <- integrate(x_state, DX[1]) the true one (k_mpc_finish)."""
    from oracle import rbd
    R, lay, P, bo = _start("go2", dyn, {})
    M = rbd.ModelArrays(R.model)
    Z = _noise(lay)
    bo.mpc_set_disturbance(state_noise=Z)
    o, werr, serr = lay.poff["x_init"][0], 0.0, 0.0
    for k in range(STEPS):
        before = bo.mpc_state()
        bo.mpc_step(k)
        xi = bo.get_params()[:, o:o + lay.nx]
        after = bo.mpc_state()
        X = bo.get_x()
        for b in range(B):
            werr = max(werr, np.abs(xi[b] - _integrate_state(M, R, dyn, before[b], Z[b])).max())
            dx1 = X[b, lay.x_off[1]:lay.x_off[1] + lay.ndx]
            serr = max(serr, np.abs(after[b] - _integrate_state(M, R, dyn, before[b], dx1)).max())
    print("noise, nominal plant", dyn, "x_init error", f"{werr:.2e}", "state error", f"{serr:.2e}")
    assert werr < QV_BAR and serr < QV_BAR, (werr, serr)
    bo.close()


def test_plant_inside_the_graph():
    """OSQP path: the plant kernel is part of the captured step.  States bit-identical to eager
    launches; new wrench values replay the same graph; a change of the plant setting re-captures
    once."""
    W0, W1 = _wrench(B, 5), _wrench(B, 6)
    runs = []
    for graph in (False, True):
        _, _, _, bo = _start("go2", "whole_body_rnea", {}, debug_paths=() if graph else ("no_mpc_graph",))
        bo.mpc_set_plant("aba", 1)
        bo.mpc_set_disturbance(base_wrench=W0)
        infos = []

        def before_step(k, bo=bo):
            if k == 2:
                bo.mpc_set_disturbance(base_wrench=W1)
            if k == 3:
                bo.mpc_set_plant("aba", 4)

        states = []
        for k in range(5):
            before_step(k)
            bo.mpc_step(k)
            states.append(bo.mpc_state())
            infos.append(bo.mpc_graph_info())
        runs.append((states, bo.get_x(), infos))
        bo.close()
    (es, ex, ei), (gs, gx, gi) = runs
    for k in range(5):
        assert np.array_equal(es[k], gs[k]), k
    assert np.array_equal(ex, gx)
    assert ei[-1] == {"captures": 0, "replays": 0, "eager_fallback": 1}, ei
    # step 0 eager (first sighting), step 1 captures, step 2 replays with the new wrench values,
    # step 3 eager (the setting changed), step 4 captures again
    assert [i["captures"] for i in gi] == [0, 1, 1, 1, 2], gi
    assert [i["replays"] for i in gi] == [0, 1, 2, 2, 3], gi
    assert all(i["eager_fallback"] == 0 for i in gi), gi


def test_plant_after_the_interior_point_solve():
    """The interior-point step ends in the same plant kernel."""
    R, lay, P, bo = _start("go2", "whole_body_rnea", {}, nodes=20, batch=2, solver="fatrop")
    W = _wrench(2)
    bo.mpc_set_plant("aba", 4)
    bo.mpc_set_disturbance(base_wrench=W)
    try:
        _run_plant(bo, R, lay, P, W, 4, steps=2, tag="fatrop")
    finally:
        bo.close()
