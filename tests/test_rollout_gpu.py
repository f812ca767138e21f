"""The rollout of the device MPC loop on the MI355X: the on-device log (k_mpc_record), the outcome
metrics, time-windowed pushes (pl_mpc_set_push) and pl_mpc_run.

Everything here is an identity, so every comparison is bit for bit (as uint64 words, so that
a NaN equals itself): the log against the per-step blocking reads of the same run, a logged run
against an unlogged one, pl_mpc_run against stepwise calls, the push schedule against host
mpc_set_disturbance calls at the same steps.  The device's metrics are compared with the numpy twin
(tests/rollout_ref.py) applied to the device's own log, at the bars of tests/test_rollout_host.py:
integers, max_dz and max_viol exact, min_cz within 1e-15.

Shapes: the plant tests' (tests/test_plant_gpu.py): N = 6, batch 3, 5 steps, synthetic problems,
each with its own dt_min."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime)

import rollout_ref as rr
from test_plant_gpu import _start, _wrench

pytestmark = pytest.mark.gpu

N, B, STEPS = 6, 3, 5
DZ_TOL = [1e30, 1e-9, np.finfo(np.float64).max]   # never (finite), the first move, what NULL stands for
CZ_MIN = [-1e30, -1e30, -np.finfo(np.float64).max]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _handle(rname="go2", dyn="whole_body_rnea", plant=None, contact=False, solver=None):
    R, lay, P, bo = _start(rname, dyn, {}, solver=solver)
    if plant is not None:
        bo.mpc_set_plant("aba", plant)
    if contact:
        xs = bo.mpc_state()
        bo.mpc_set_contact(bo.contact_defaults(kp=40.0, kd=1.0), bo.ground_under_feet(xs, 0.005))
    return lay, bo


def _reads(bo, lay):
    """The blocking per-step reads, as one log row's fields [B][width]."""
    o, w = lay.poff["x_init"][0], lay.nx
    dl, st, c = bo.mpc_download(), bo.mpc_stats(), bo.mpc_get_contact()
    nu0 = lay.nu[0]
    return {"x_init": bo.get_params()[:, o:o + w], "u0": dl[:, :nu0],
            "stats": np.stack([st[k].astype(np.float64) for k in rr.STATS], -1), "x_state": bo.mpc_state(),
            "ground_f": c["forces"].reshape(B, -1), "anchor_active": (c["anchors"][:, :, 2] != 0).astype(np.float64),
            "dl_state": dl[:, nu0:]}


def _run(bo, k0, steps):
    """mpc_run, then the handle's stream drained.  Two handles never have steps in flight at once
    here, as in the plant and contact tests: k_plant needs 24 KB of scratch per lane, which the
    runtime provides per hardware queue, and two queues asking for it at the same moment is a
    load these tests are not about."""
    bo.mpc_run(k0, steps)
    bo.sync()


def _stepwise(bo, lay, steps=STEPS, k0=0):
    rows = []
    for k in range(k0, k0 + steps):
        bo.mpc_step(k)
        rows.append(_reads(bo, lay))
    return rows


def _check_metrics(bo, log, ks, z_ref, qoff=0, dz_tol=DZ_TOL, cz_min=CZ_MIN):
    met = bo.mpc_metrics()
    for b in range(B):
        want = rr.metrics(ks, log["x_state"][:, b], log["stats"][:, b], z_ref[b], dz_tol[b], cz_min[b], qoff)
        got = {k: met[k][b] for k in met}
        print(f"problem {b}: device {got}")
        rr.compare(got, want, who=b)
    return met


VARIANTS = [("go2", "whole_body_rnea", None, False, None, STEPS),
            ("go2", "whole_body_rnea", 2, True, None, STEPS),
            ("b2g", "whole_body_rnea", 2, False, None, STEPS),
            ("go2", "centroidal_vel", None, False, None, STEPS),
            ("go2", "whole_body_rnea", None, False, "fatrop", 2)]
IDS = ["go2-rnea-nominal", "go2-rnea-aba-contact", "b2g-rnea-aba", "go2-cv-nominal", "go2-rnea-ip"]


@pytest.mark.parametrize("rname,dyn,plant,contact,solver,steps", VARIANTS, ids=IDS)
def test_log_equals_the_per_step_reads(rname, dyn, plant, contact, solver, steps):
    """The log read once at the end is, field by field, what the blocking reads returned after
    each step of the same run; the device's metrics are the twin's over that log."""
    lay, bo = _handle(rname, dyn, plant, contact, solver)
    try:
        qoff = 6 if dyn == "centroidal_vel" else 0
        if plant is not None:
            bo.mpc_set_disturbance(base_wrench=_wrench(B))
        z_ref = bo.mpc_state()[:, qoff + 2].copy()
        bo.mpc_log_start(capacity=steps, every=1, dz_tol=DZ_TOL, cz_min=CZ_MIN)
        rows = _stepwise(bo, lay, steps)
        log = bo.mpc_log_read()
        sz = bo.mpc_log_sizes()
        assert (sz["recorded"], sz["dropped"], sz["capacity"], sz["every"]) == (steps, 0, steps, 1)
        for f in rr.FIELDS:
            want = np.stack([r[f] for r in rows])
            assert log[f].shape == (steps, B, sz[f]["width"]) == want.shape, f
            assert _same(log[f], want), (f, np.abs(log[f] - want).max())
        assert all(_same(r["dl_state"], r["x_state"]) for r in rows)
        assert not _same(log["x_state"][0], log["x_state"][-1])   # the loop moved
        if contact:
            assert log["ground_f"].any() and log["anchor_active"].any()
        else:
            assert not log["ground_f"].any() and not log["anchor_active"].any()
        met = _check_metrics(bo, log, range(steps), z_ref, qoff)
        assert np.all(met["steps"] == steps)
        # problem 1's tolerance catches the first step whose logged height left z_ref
        moved = np.nonzero(np.abs(log["x_state"][:, 1, qoff + 2] - z_ref[1]) > 1e-9)[0]
        assert met["first_out"][1] == (moved[0] if len(moved) else -1)
        assert met["first_out"][0] == -1 and met["first_out"][2] == -1
        # slots beyond `recorded` are refused
        from pinoloco import _lib
        with pytest.raises(_lib.PinolocoError, match="recorded"):
            bo.mpc_log_read(1, steps)
        assert bo.mpc_log_device()
    finally:
        bo.close()


def test_logging_changes_nothing_and_never_recaptures():
    """The states of a logged run equal an unlogged run's on a second handle, and the step's graph is
    captured once across log_start -> steps -> log_stop -> steps -> set_push -> steps."""
    lay, a = _handle(plant=2)
    _, b = _handle(plant=2)
    try:
        sa, sb, caps = [], [], []
        for k in range(6):
            if k == 2:
                a.mpc_log_start(capacity=2, every=1)
            if k == 4:
                a.mpc_log_stop()
            if k == 5:   # an empty window: the schedule is set and pushes nothing
                a.mpc_set_push(0, 0, _wrench(B))
            a.mpc_step(k)
            sa.append(a.mpc_state())
            caps.append(a.mpc_graph_info())
        for k in range(6):
            b.mpc_step(k)
            sb.append(b.mpc_state())
        assert _same(np.stack(sa), np.stack(sb))
        # step 0 eager (first sighting), step 1 captures, everything after replays
        assert [c["captures"] for c in caps] == [0, 1, 1, 1, 1, 1], caps
        assert [c["replays"] for c in caps] == [0, 1, 2, 3, 4, 5], caps
        assert all(c["eager_fallback"] == 0 for c in caps), caps
        assert b.mpc_graph_info()["captures"] == 1
        log = a.mpc_log_read()
        assert _same(log["x_state"], np.stack(sa[2:4]))
        assert a.mpc_metrics()["steps"].tolist() == [2] * B
        assert a.mpc_log_sizes()["recorded"] == 2
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("parts", [[(0, 5)], [(0, 2), (2, 3)]], ids=["run-0-5", "run-0-2-then-2-3"])
def test_run_equals_stepwise(parts):
    lay, a = _handle(plant=2)
    _, b = _handle(plant=2)
    try:
        for bo in (a, b):
            bo.mpc_set_disturbance(base_wrench=_wrench(B))
            bo.mpc_log_start(capacity=STEPS, dz_tol=DZ_TOL, cz_min=CZ_MIN)
        for k0, steps in parts:
            a.mpc_run(k0, steps)
        a.sync()
        for k in range(STEPS):
            b.mpc_step(k)
        la, lb = a.mpc_log_read(), b.mpc_log_read()
        for f in rr.FIELDS:
            assert la[f].shape[0] == STEPS and _same(la[f], lb[f]), f
        ma, mb = a.mpc_metrics(), b.mpc_metrics()
        for k in ma:
            assert _same(ma[k].astype(np.float64), mb[k].astype(np.float64)), k
        assert _same(a.mpc_state(), b.mpc_state())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("window", [(1, 2), (0, 0), (0, 5)], ids=["1-2", "0-0", "0-5"])
def test_push_windows_equal_host_disturbances(window):
    """The schedule on the device against mpc_set_disturbance calls from the host at the same steps."""
    from pinoloco import _lib
    lay, a = _handle(plant=2)
    _, b = _handle(plant=2)
    try:
        W = _wrench(B)
        k0 = np.array([window[0], window[0], 0], dtype=np.int32)   # problem 2: its own window [0, 1)
        k1 = np.array([window[1], window[1], 1], dtype=np.int32)
        a.mpc_set_push(k0, k1, W)
        with pytest.raises(_lib.PinolocoError, match="push schedule"):
            a.mpc_set_disturbance(base_wrench=W)
        a.mpc_set_disturbance(state_noise=None)   # without a wrench: allowed, the schedule stays
        a.mpc_log_start(capacity=STEPS)
        _run(a, 0, STEPS)
        sb = []
        for k in range(STEPS):
            on = (k0 <= k) & (k < k1)
            b.mpc_set_disturbance(base_wrench=np.where(on[:, None], W, 0.0))
            b.mpc_step(k)
            sb.append(b.mpc_state())
        sb = np.stack(sb)
        assert _same(a.mpc_log_read()["x_state"], sb)
        a.mpc_set_push()
        a.mpc_set_disturbance(base_wrench=W)   # the schedule is off: accepted again
    finally:
        a.close()
        b.close()


def test_push_moves_the_state():
    """A pushed problem leaves the unpushed trajectory exactly at its window; the others never do."""
    lay, a = _handle(plant=2)
    _, b = _handle(plant=2)
    try:
        a.mpc_set_push([1, 0, 0], [2, 0, 0], _wrench(B))
        a.mpc_log_start(capacity=STEPS)
        _run(a, 0, STEPS)
        b.mpc_log_start(capacity=STEPS)
        _run(b, 0, STEPS)
        xa, xb = a.mpc_log_read()["x_state"], b.mpc_log_read()["x_state"]
        assert _same(xa[:, 1:], xb[:, 1:]) and _same(xa[0, 0], xb[0, 0])
        assert not _same(xa[1, 0], xb[1, 0])
    finally:
        a.close()
        b.close()


def test_capacity_and_stride():
    """every = 2 with capacity = 2 over 5 steps: steps 0 and 2 recorded, one dropped, metrics of all
    five; capacity 0 keeps the metrics only; a restart reuses the buffers and resets the cursor.
    The reference is a second handle that logs every one of the same 8 steps."""
    lay, a = _handle(plant=2)
    _, b = _handle(plant=2)
    try:
        b.mpc_log_start(capacity=STEPS + 3)
        _run(b, 0, STEPS + 3)
        full = b.mpc_log_read()
        lb, lb2 = ({f: full[f][:STEPS] for f in rr.FIELDS}, {f: full[f][STEPS:] for f in rr.FIELDS})
        z_ref = a.mpc_state()[:, 2].copy()
        a.mpc_log_start(capacity=2, every=2, dz_tol=DZ_TOL, cz_min=CZ_MIN)
        _run(a, 0, STEPS)
        la = a.mpc_log_read()
        sz = a.mpc_log_sizes()
        assert (sz["recorded"], sz["dropped"], sz["capacity"], sz["every"]) == (2, 1, 2, 2)
        for f in rr.FIELDS:
            assert _same(la[f], lb[f][[0, 2]]), f
        assert _same(a.mpc_log_read(1, 1)["x_state"], lb["x_state"][2:3])
        met = _check_metrics(a, lb, range(STEPS), z_ref)   # the metrics saw all five steps
        assert met["steps"].tolist() == [STEPS] * B
        # metrics only, on the running loop: z_ref is the state now
        z_ref = a.mpc_state()[:, 2].copy()
        assert _same(z_ref, lb["x_state"][-1][:, 2])
        a.mpc_log_start(capacity=0, dz_tol=DZ_TOL, cz_min=CZ_MIN)
        _run(a, STEPS, 3)
        sz = a.mpc_log_sizes()
        assert (sz["recorded"], sz["dropped"], sz["capacity"]) == (0, 3, 0)
        assert a.mpc_log_read()["x_state"].shape == (0, B, lay.nx)
        assert a.mpc_log_device() is None
        met = _check_metrics(a, lb2, range(STEPS, STEPS + 3), z_ref)
        assert met["steps"].tolist() == [3] * B
    finally:
        a.close()
        b.close()
