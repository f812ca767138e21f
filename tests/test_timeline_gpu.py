"""Gait and command timelines of the device MPC loop on the MI355X (pl_mpc_set_timeline,
k_mpc_prepare with a timeline, csrc/timeline.h).

What k_mpc_prepare writes is compared with pl_mpc_timeline_host (the same header on the host) and
with the numpy twin (tests/timeline_ref.py) at the bars of tests/test_timeline_host.py: the
governing keyframe, gait scalars, schedules, warm start and held or clamped commands bit for bit,
a ramped command within 2**-51 (|c_s| + |c_{s+1}|).  Everything else is an identity between two
runs on the device and is compared bit for bit, as uint64 words (tests/test_rollout_gpu.py).

Shapes: Go2 whole_body_rnea, N = 6, batch 4 (3 where a test names three gaits), at most 6 steps,
synthetic problems, each with its own dt_min; one B2G rnea and one Go2 centroidal_vel case.

Horizon: the device-against-device identities run on the synthetic geometric horizon (dt_min ...
0.08 s).  Where the device's schedule is compared with the host's or the twin's, the problems get
dt_max = dt_min (each its own), a uniform horizon: the node times are t_{i+1} = fma(dt_min,
gamma^i, t_i) with gamma = pow(dt_max / dt_min, 1 / (N - 1)), and the device's pow and the host's are
two libraries that are each within an ulp or so of the true value but not of each other.  On the
geometric horizon that shows: at k = 4 of the mixed timeline problem 0's node times from node 3 on
differ by one ulp between the MI355X and the host (swing phases 0x1.ac07ad17b14e8p-2 against
0x1.ac07ad17b14dap-2), with every input and every other operation equal.  pow(1, y) is exactly 1 in
both, so on a uniform horizon the bit-for-bit bar measures the timeline code and the clock, which
is what it is set for; the fused node-time step is still exercised, with gamma^i = 1."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime)

import rollout_ref as rr
import timeline_ref as tr
from conftest import make_robot
from test_timeline_host import MIXED, MIXED_EE, SINGLE, kf

pytestmark = pytest.mark.gpu

N, B, STEPS = 6, 4, 5


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _start(rname="go2", dyn="whole_body_rnea", batch=B, gait="trot", period=0.8, solver=None, plant=None, contact=False,
           uniform=False):
    """A handle ready for mpc_step(0) on synthetic problems 0..batch-1, each with its own dt_min; the
    handle's one gait is (gait, period), and the parameters carry that gait's scalars.  uniform:
    dt_max = dt_min per problem (the module docstring says where and why)."""
    from pinoloco.gait import GaitSequence
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import DT_MIN, build_batch
    R = make_robot(rname)
    lay, P, X, XS, T0 = build_batch(R, dyn, N, batch, 0)
    P = P.copy()
    P[:, lay.poff["dt_min"][0]] = DT_MIN * (1.0 + 0.1 * np.arange(batch))
    if uniform:
        P[:, lay.poff["dt_max"][0]] = P[:, lay.poff["dt_min"][0]]
    gs = GaitSequence(gait, period)
    P[:, lay.poff["n_contacts"][0]] = gs.n_contacts
    P[:, lay.poff["swing_period"][0]] = gs.swing_period
    bo = BatchedOCP(R, dyn, N, batch=batch, device=0, gait_type=gait, gait_period=period)
    if solver is not None:
        bo.set_solver(solver)
        bo.set_ip_settings()
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    bo.mpc_setup(XS, T0)
    if plant is not None:
        bo.mpc_set_plant("aba", plant)
    if contact:
        bo.mpc_set_contact(bo.contact_defaults(kp=40.0, kd=1.0), bo.ground_under_feet(bo.mpc_state(), 0.005))
    return R, lay, P, X, T0, bo


def _run(bo, k0, steps):
    """mpc_run, then the handle's stream drained: two handles never have steps in flight at once
    (tests/test_rollout_gpu.py _run gives the reason)."""
    bo.mpc_run(k0, steps)
    bo.sync()


def _logged_run(bo, steps=STEPS):
    bo.mpc_log_start(capacity=steps)
    _run(bo, 0, steps)
    return bo.mpc_log_read()


def _own_commands(lay, P, b, k_start=0, gait="trot", period=0.8, **kw):
    """A keyframe that repeats the commands problem b already has in its parameters."""
    from pinoloco.ocp import BatchedOCP
    get = lambda n: P[b, lay.poff[n][0]:lay.poff[n][0] + lay.poff[n][1]].copy()
    return BatchedOCP.keyframe(k_start, gait, period, get("base_vel_des"), get("ext_force_des"), get("arm_vel_des"), **kw)


def _check_prepared(bo, R, lay, keys, k, T0, p_in, x_in, worst):
    """The device's p, x and timeline state after the prepare launch of step k against the host
    step and the twin, both run on the device's p and x from before the launch."""
    p, x, st = bo.get_params(), bo.get_x(), bo.mpc_timeline_state()
    for b in range(bo.batch):
        want = tr.prepare(R, lay, keys[b], k, T0[b], p_in[b], x_in[b])
        ph, xh, seg = bo.mpc_timeline_host(k, T0[b], keys[b], p_in[b], x_in[b])
        who = (k, b)
        worst[0] = max(worst[0], tr.compare(p[b], want, lay, R, who=who + ("twin",)))
        worst[0] = max(worst[0], tr.compare(p[b], dict(want, p=ph), lay, R, who=who + ("host",)))
        assert _same(x[b], want["x"]) and _same(x[b], xh), who
        assert (st["seg"][b], st["gait_type"][b]) == (want["seg"], want["gait_type"]) == (seg, want["gait_type"]), who
        assert st["gait_period"][b] == want["gait_period"], who
        dev = np.abs(st["commands"][b] - want["commands"])
        assert np.all(dev <= want["bar"]), (who, dev, want["bar"])
    return p, x


# ---------------------------------------------------------------- 1. prepare parity
def _mixed_keys(batch, ee=False):
    """Per-problem gaits, periods and counts, ramps, a clamped start and t_shift."""
    base = MIXED_EE if ee else MIXED
    keys = [base, SINGLE, base[:2], [kf(0, "stand", 0.5, 0.2), kf(4, "walk", 0.6, -0.1, ramp=1, t_shift=0.04),
                                     kf(5, "trot", 0.9, 0.3)]]
    return keys[:batch]


@pytest.mark.parametrize("rname,dyn", [("go2", "whole_body_rnea"), ("b2g", "whole_body_rnea"), ("go2", "centroidal_vel")],
                         ids=["go2-rnea", "b2g-rnea", "go2-cv"])
def test_prepare_equals_host_and_twin(rname, dyn):
    from pinoloco import _lib
    R, lay, P, X, T0, bo = _start(rname, dyn, uniform=True)
    try:
        keys = _mixed_keys(B, ee=rname == "b2g")
        if rname == "go2" and dyn == "whole_body_rnea":
            # as a structured array: counts below n_key, NaN and out-of-range integers in the padding
            arr, cnt = bo._keyframes(keys, B)
            wide = np.zeros((B, arr.shape[1] + 2), dtype=_lib.timeline_dtype)
            wide["gait_period"], wide["base_vel_des"], wide["k_start"], wide["gait_type"] = np.nan, np.inf, -9, 77
            for b in range(B):
                wide[b, :cnt[b]] = arr[b, :cnt[b]]
            bo.mpc_set_timeline(wide, count=cnt)
            assert bo.mpc_get_timeline() == {"on": True, "n_key": arr.shape[1] + 2}
        else:
            bo.mpc_set_timeline(keys)
        worst = [0.0]
        p_in, x_in = bo.get_params(), bo.get_x()
        assert _same(x_in, X)
        for k in (0, 1, 2, 3, 4, 7, 9, 12):
            bo.debug_mpc_prepare(k)
            p_out, x_out = _check_prepared(bo, R, lay, keys, k, T0, p_in, x_in, worst)
            if k == 0:
                assert _same(x_out, X)        # step 0 keeps the initial guess
            p_in, x_in = p_out, x_out
        print(f"{rname} {dyn}: worst ramped command deviation {worst[0]:.3f} of its bar")
    finally:
        bo.close()


# ---------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("plant", [None, 2], ids=["nominal", "aba-contact"])
def test_own_gait_and_commands_change_nothing(plant):
    """One keyframe equal to the handle's gait and the commands already in p: x_init, u0, the stats
    and x_state of 5 steps are those of the same setup without a timeline."""
    R, lay, P, X, T0, a = _start(plant=plant, contact=plant is not None)
    _, _, _, _, _, b = _start(plant=plant, contact=plant is not None)
    try:
        a.mpc_set_timeline([[_own_commands(lay, P, i)] for i in range(B)])
        la = _logged_run(a)
        lb = _logged_run(b)
        for f in rr.FIELDS:
            assert la[f].shape[0] == STEPS and _same(la[f], lb[f]), f
        assert not _same(la["x_state"][0], la["x_state"][-1])
        assert _same(a.get_params(), b.get_params()) and _same(a.get_x(), b.get_x())
        assert a.mpc_timeline_state()["seg"].tolist() == [0] * B
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3. per-problem gait = per-handle gait
GAITS3 = [("trot", 0.8), ("walk", 0.6), ("stand", 0.5)]


def test_per_problem_gait_equals_per_handle_gait():
    """Handle T walks gait g_b in problem b from k = 0; handles H_g walk g in every problem.  After 5
    steps row b of T is row b of H_{g_b}."""
    R, lay, P, X, T0, t = _start(batch=3)
    try:
        t.mpc_set_timeline([[_own_commands(lay, P, b, 0, g, per)] for b, (g, per) in enumerate(GAITS3)])
        lt = _logged_run(t)
        pt, xt = t.get_params(), t.get_x()
    finally:
        t.close()
    for b, (g, per) in enumerate(GAITS3):
        _, _, _, _, _, h = _start(batch=3, gait=g, period=per)
        try:
            lh = _logged_run(h)
            for f in rr.FIELDS:
                assert _same(lt[f][:, b], lh[f][:, b]), (g, f)
            assert _same(pt[b], h.get_params()[b]) and _same(xt[b], h.get_x()[b]), g
            # the other rows walk another gait: they differ
            assert not _same(lt["x_state"][:, (b + 1) % 3], lh["x_state"][:, (b + 1) % 3]), g
        finally:
            h.close()


# ---------------------------------------------------------------- 4. a switch does not leak
K_S = 3
SWITCH_TO = [("walk", 0.6, 0.0), ("stand", 0.5, 0.0), ("trot", 0.5, 0.07), ("walk", 0.9, 0.02)]


def _switch_keys(lay, P):
    return [[_own_commands(lay, P, b), _own_commands(lay, P, b, K_S, g, per, t_shift=ts)]
            for b, (g, per, ts) in enumerate(SWITCH_TO)]


def test_a_switch_does_not_leak_backwards():
    """T switches trot 0.8 -> g2 at k = 3.  The rows of steps 0..2 are the constant-trot handle's;
    from step 3 on the parameters read after the step are the twin's for g2, segment 1."""
    R, lay, P, X, T0, t = _start(uniform=True)
    _, _, _, _, _, h = _start(uniform=True)
    try:
        keys = _switch_keys(lay, P)
        t.mpc_set_timeline(keys)
        t.mpc_log_start(capacity=STEPS)
        for k in range(STEPS):
            t.mpc_step(k)
            p, st = t.get_params(), t.mpc_timeline_state()
            assert st["seg"].tolist() == [int(k >= K_S)] * B, k
            for b in range(B):
                want = tr.prepare(R, lay, keys[b], k, T0[b], p[b])
                tr.compare(p[b], want, lay, R, who=(k, b))
                assert st["gait_type"][b] == want["gait_type"] and st["gait_period"][b] == want["gait_period"]
                assert p[b, lay.poff["n_contacts"][0]] == (2.0 if k < K_S else {"walk": 3.0, "stand": 4.0, "trot": 2.0}[
                    SWITCH_TO[b][0]])
        lt = t.mpc_log_read()
        lh = _logged_run(h)
        for f in rr.FIELDS:
            assert _same(lt[f][:K_S], lh[f][:K_S]), f
        # the step of the switch plans from the same state and then walks another gait
        assert _same(lt["x_init"][K_S], lh["x_init"][K_S])
        for b in range(B):
            assert not _same(lt["x_state"][K_S:, b], lh["x_state"][K_S:, b]), b
    finally:
        t.close()
        h.close()


# ---------------------------------------------------------------- 5. no re-capture, refusals keep the timeline
def test_set_timeline_never_recaptures_and_refusals_keep_it():
    from pinoloco import _lib
    R, lay, P, X, T0, bo = _start()
    try:
        caps = []
        for k in range(6):
            if k == 2:    # on
                bo.mpc_set_timeline(_switch_keys(lay, P))
            if k == 3:    # a refusal in between leaves it as it is
                with pytest.raises(_lib.PinolocoError, match="problem 2, keyframe 1"):
                    bo.mpc_set_timeline([[_own_commands(lay, P, b), _own_commands(lay, P, b, 0 if b == 2 else 5)]
                                         for b in range(B)])
                assert bo.mpc_get_timeline() == {"on": True, "n_key": 2}
            if k == 4:    # changed, with another n_key: the keyframe buffer is reallocated
                bo.mpc_set_timeline([MIXED] * B)
                assert bo.mpc_get_timeline() == {"on": True, "n_key": 4}
            if k == 5:    # off
                bo.mpc_set_timeline(None)
                assert bo.mpc_get_timeline() == {"on": False, "n_key": 0}
            bo.mpc_step(k)
            if k == 3:
                st = bo.mpc_timeline_state()
                assert st["seg"].tolist() == [1] * B and st["gait_period"].tolist() == [s[1] for s in SWITCH_TO]
            if k == 4:
                assert bo.mpc_timeline_state()["gait_type"].tolist() == [1] * B   # MIXED at k = 4: walk
            caps.append(bo.mpc_graph_info())
        # step 0 eager (first sighting), step 1 captures, everything after replays
        assert [c["captures"] for c in caps] == [0, 1, 1, 1, 1, 1], caps
        assert [c["replays"] for c in caps] == [0, 1, 2, 3, 4, 5], caps
        assert all(c["eager_fallback"] == 0 for c in caps), caps
        with pytest.raises(_lib.PinolocoError, match="no timeline"):
            bo.mpc_timeline_state()
    finally:
        bo.close()


# ---------------------------------------------------------------- 6. mpc_run = stepwise calls
def test_run_equals_stepwise_under_a_timeline():
    R, lay, P, X, T0, a = _start(plant=2)
    _, _, _, _, _, b = _start(plant=2)
    try:
        keys = _mixed_keys(B)
        for bo in (a, b):
            bo.mpc_set_timeline(keys)
            bo.mpc_log_start(capacity=STEPS + 1)
        a.mpc_run(0, 2)
        a.mpc_run(2, STEPS - 1)
        a.sync()
        for k in range(STEPS + 1):
            b.mpc_step(k)
        la, lb = a.mpc_log_read(), b.mpc_log_read()
        for f in rr.FIELDS:
            assert la[f].shape[0] == STEPS + 1 and _same(la[f], lb[f]), f
        assert _same(a.get_params(), b.get_params()) and _same(a.mpc_state(), b.mpc_state())
        sa, sb = a.mpc_timeline_state(), b.mpc_timeline_state()
        assert all(_same(sa[k].astype(np.float64), sb[k].astype(np.float64)) for k in sa)
        assert sa["seg"].tolist() == [tr.segment(kb, STEPS) for kb in keys]
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 7. the interior-point solver
def test_interior_point_loop_follows_the_timeline():
    """Two steps with a switch at k = 1: the parameters are the twin's, and the statuses of
    mpc_run are those of stepwise calls."""
    R, lay, P, X, T0, a = _start(solver="fatrop", uniform=True)
    _, _, _, _, _, b = _start(solver="fatrop", uniform=True)
    try:
        keys = [[_own_commands(lay, P, i), _own_commands(lay, P, i, 1, g, per, t_shift=ts)]
                for i, (g, per, ts) in enumerate(SWITCH_TO)]
        for bo in (a, b):
            bo.mpc_set_timeline(keys)
            bo.mpc_log_start(capacity=2)
        _run(a, 0, 2)
        for k in range(2):
            b.mpc_step(k)
            p = b.get_params()
            for i in range(B):
                tr.compare(p[i], tr.prepare(R, lay, keys[i], k, T0[i], p[i]), lay, R, who=(k, i))
            assert b.mpc_timeline_state()["seg"].tolist() == [k] * B
        la, lb = a.mpc_log_read(), b.mpc_log_read()
        assert _same(la["stats"][:, :, 0], lb["stats"][:, :, 0])
        for f in rr.FIELDS:
            assert _same(la[f], lb[f]), f
        assert _same(a.get_params(), b.get_params())
        assert np.all(np.isfinite(la["x_state"]))
    finally:
        a.close()
        b.close()
