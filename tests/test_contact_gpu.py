"""Ground contact and joint PD of the MPC plant (pl_mpc_set_contact, k_plant.hip's contact
instantiation, plant.h) on the MI355X.

The numpy twin of tests/contact_ref.py is applied, teacher-forced per step, to mpc_state() and
mpc_get_contact() before the step, with the tau and forces of node 0 and the joint q, v of node 1
that the device's retract returns after the step (the retract has its own tests,
tests/test_retract_gpu.py, so the bars here measure the plant).  Inputs, coverage conditions and
bars are those of tests/test_contact_host.py (contact_ref.case_inputs, check_log, bars): every
branch decision of the twin clear of round-off by 1e-9, each of the five events seen, state at
1e-10 x max(1, max |a|), ground forces at (k_n + k_t + d_n + d_t) x 1e-12, anchors at
1e-12 x (2 + d_t / k_t).

Shapes: tests/test_plant_gpu.py's: N = 6, batch 3, synthetic problems with their own dt_min,
three MPC steps; before step 2 the ground under one foot is lowered by 2 cm."""
import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libpinoloco.so, so both share one HIP runtime)

import contact_ref as cr
from test_plant_gpu import _loop, _start, _wrench

pytestmark = pytest.mark.gpu

N, B, STEPS = 6, 3, 3
VARIANTS = [("go2", "whole_body_rnea", 1), ("go2", "whole_body_rnea", 4), ("go2", "whole_body_rnea", 16),
            ("go2", "whole_body_acc", 1), ("go2", "whole_body_acc", 4),
            ("go2", "whole_body_aba", 1), ("go2", "whole_body_aba", 4),
            ("b2g", "whole_body_rnea", 1), ("b2g", "whole_body_rnea", 4)]


def _contact_start(rname, dyn, substeps, **kw):
    R, lay, P, bo = _start(rname, dyn, {}, **kw)
    prm, GZ = cr.case_inputs(bo, bo.mpc_state())
    bo.mpc_set_plant("aba", substeps)
    bo.mpc_set_contact(prm, GZ)
    return R, lay, P, bo, prm, GZ


def _run_contact(bo, R, lay, P, prm, GZ, W, substeps, steps=STEPS, lower_at=2, host=True, tag=""):
    """`steps` closed-loop steps, each checked against the twin (and the host entry) from the
    device's own state and anchors before the step.  Returns the events seen."""
    from oracle import rbd
    M = rbd.ModelArrays(R.model)
    nb, nq, nv = P.shape[0], R.nq, R.nv
    seen, worst = set(), {"x": 0.0, "f": 0.0, "anchor": 0.0, "host": 0.0}
    GZ = GZ.copy()
    for k in range(steps):
        before, cb = bo.mpc_state(), bo.mpc_get_contact()
        assert cb["on"]
        if k == lower_at:  # under each problem's first standing foot (the first foot if none stands)
            feet = np.argmax(cb["anchors"][:, :, 2], axis=1)
            GZ[np.arange(nb), feet] -= 0.02
            bo.mpc_set_contact(prm, GZ)
        bo.mpc_step(k)
        ret = bo.retract(2)
        after, ca = bo.mpc_state(), bo.mpc_get_contact()
        X, Pk = bo.get_x(), bo.get_params()
        assert np.all(np.isfinite(after)), k
        for b in range(nb):
            c = cr.one(prm, b)
            want = cr.contact_plant(M, R.foot_frames, R.ext_force_frame, nq, before[b], ret["tau"][b, 0],
                                    ret["forces"][b, 0], ret["q"][b, 1, 7:], ret["v"][b, 1, 6:], W[b],
                                    P[b, lay.poff["dt_min"][0]], substeps, c, GZ[b], cb["anchors"][b])
            cr.check_log(want[4], seen)
            bx, bf, ba = cr.bars(c, want[3])
            got = (after[b], ca["anchors"][b], ca["forces"][b])
            ex, ea, ef = (np.abs(got[i] - want[i]).max() for i in range(3))
            print(f"contact {tag} step {k} problem {b}: state {ex:.2e} / {bx:.2e}, forces {ef:.2e} / {bf:.2e}, "
                  f"anchors {ea:.2e} / {ba:.2e}")
            worst = dict(worst, x=max(worst["x"], ex / bx), f=max(worst["f"], ef / bf), anchor=max(worst["anchor"], ea / ba))
            assert ex < bx and ef < bf and ea < ba, (k, b, (ex, bx), (ef, bf), (ea, ba))
            if host:  # the same step through the host entry, to the same bars
                hs = bo.mpc_plant_host(Pk[b], X[b], before[b], substeps, W[b], c, GZ[b], cb["anchors"][b])
                hx, ha, hf = (np.abs(got[i] - hs[i]).max() for i in range(3))
                worst["host"] = max(worst["host"], hx / bx, hf / bf, ha / ba)
                assert hx < bx and hf < bf and ha < ba, (k, b, (hx, bx), (hf, bf), (ha, ba))
    print("contact errors / bar", tag, f"substeps={substeps}", {k: f"{v:.2e}" for k, v in worst.items()}, sorted(seen))
    return seen


@pytest.mark.parametrize("rname,dyn,substeps", VARIANTS, ids=[f"{r}-{d}-{s}" for r, d, s in VARIANTS])
def test_contact_matches_twin_and_host(rname, dyn, substeps):
    """Device against the twin and against the host entry: tau from u (rnea, aba) or from the RNEA
    rows (acc), B2G's external-force frame keeping its command, under a distinct wrench per problem."""
    R, lay, P, bo, prm, GZ = _contact_start(rname, dyn, substeps)
    W = _wrench(B)
    bo.mpc_set_disturbance(base_wrench=W)
    try:
        seen = _run_contact(bo, R, lay, P, prm, GZ, W, substeps, tag=f"{rname}-{dyn}")
    finally:
        bo.close()
    assert seen == set(cr.EVENTS), seen


def test_set_contact_round_trips():
    R, lay, P, bo, prm, GZ = _contact_start("go2", "whole_body_rnea", 2)
    assert bo.mpc_get_contact()["on"] and bo.mpc_get_plant() == ("aba", 2)
    bo.mpc_set_contact()
    c = bo.mpc_get_contact()
    assert not c["on"] and not c["anchors"].any() and not c["forces"].any()
    bo.mpc_set_plant("nominal")  # stored while nominal, in effect once "aba" is selected
    bo.mpc_set_contact(prm, GZ)
    assert bo.mpc_get_contact()["on"]
    bo.mpc_step(0)
    assert not bo.mpc_get_contact()["anchors"].any()  # the nominal plant touches no ground
    bo.mpc_set_plant("aba", 2)
    bo.mpc_step(1)
    assert bo.mpc_get_contact()["anchors"][:, :, 2].any()
    bo.close()


@pytest.mark.parametrize("mode", ["aba", "nominal"])
def test_contact_off_is_the_old_plant(mode):
    """Contact set and cleared again: the states of a handle that never called the new interface,
    bit for bit."""
    _, _, _, plain = _start("go2", "whole_body_rnea", {})
    R, lay, P, named, prm, GZ = _contact_start("go2", "whole_body_rnea", 2)
    named.mpc_set_contact()
    W = _wrench(B)
    for bo in (plain, named):
        bo.mpc_set_plant(mode, 2)
        bo.mpc_set_disturbance(base_wrench=W)
    a, b = _loop(plain, STEPS), _loop(named, STEPS)
    for k in range(STEPS):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(plain.get_x(), named.get_x())
    assert not named.mpc_get_contact()["anchors"].any()
    plain.close()
    named.close()


def test_problems_are_independent():
    """Another mu and ground on problem 1 alone move problem 1 alone."""
    R, lay, P, calm, prm, GZ = _contact_start("go2", "whole_body_rnea", 2)
    _, _, _, other, _, _ = _contact_start("go2", "whole_body_rnea", 2)
    prm2 = {k: v.copy() for k, v in prm.items()}
    prm2["mu"][1] = 0.4
    GZ2 = GZ.copy()
    GZ2[1] += 0.002
    other.mpc_set_contact(prm2, GZ2)
    a, b = _loop(calm, STEPS), _loop(other, STEPS)
    for k in range(STEPS):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][2], b[k][2]), k
        assert not np.array_equal(a[k][1], b[k][1]), k
    ca, cb = calm.mpc_get_contact(), other.mpc_get_contact()
    for key in ("anchors", "forces"):
        assert np.array_equal(ca[key][0], cb[key][0]) and np.array_equal(ca[key][2], cb[key][2]), key
    calm.close()
    other.close()


def test_contact_inside_the_graph():
    """OSQP path: the contact kernel is part of the captured step.  States and anchors
    bit-identical to eager launches; new parameter and ground values replay the same graph;
    switching contact off or on re-captures once."""
    runs = []
    for graph in (False, True):
        R, lay, P, bo, prm, GZ = _contact_start("go2", "whole_body_rnea", 2,
                                                debug_paths=() if graph else ("no_mpc_graph",))
        prm2 = dict(prm, mu=prm["mu"] * 0.5, kp=prm["kp"] + 5.0)
        states, anchors, infos = [], [], []
        for k in range(8):
            if k == 2:
                bo.mpc_set_contact(prm2, GZ)
            if k == 3:
                bo.mpc_set_contact(prm2, GZ - 0.003)
            if k == 4:
                bo.mpc_set_contact()
            if k == 6:
                bo.mpc_set_contact(prm, GZ)
            bo.mpc_step(k)
            states.append(bo.mpc_state())
            anchors.append(bo.mpc_get_contact()["anchors"])
            infos.append(bo.mpc_graph_info())
        runs.append((states, anchors, bo.get_x(), infos))
        bo.close()
    (es, ea, ex, ei), (gs, ga, gx, gi) = runs
    for k in range(8):
        assert np.array_equal(es[k], gs[k]) and np.array_equal(ea[k], ga[k]), k
    assert np.array_equal(ex, gx)
    assert ei[-1] == {"captures": 0, "replays": 0, "eager_fallback": 1}, ei
    # step 0 eager (first sighting), 1 captures, 2 and 3 replay with the new values, 4 eager (off),
    # 5 captures, 6 eager (on), 7 captures
    assert [i["captures"] for i in gi] == [0, 1, 1, 1, 1, 2, 2, 3], gi
    assert [i["replays"] for i in gi] == [0, 1, 2, 3, 3, 4, 4, 5], gi
    assert all(i["eager_fallback"] == 0 for i in gi), gi


def test_mpc_setup_clears_the_anchors():
    R, lay, P, bo, prm, GZ = _contact_start("go2", "whole_body_rnea", 2)
    xs0 = bo.mpc_state()
    bo.mpc_step(0)
    c = bo.mpc_get_contact()
    assert c["anchors"][:, :, 2].any() and c["forces"].any()
    bo.mpc_setup(xs0, np.zeros(B))
    c = bo.mpc_get_contact()
    assert c["on"] and not c["anchors"].any() and not c["forces"].any()
    bo.close()


def test_contact_after_the_interior_point_solve():
    """The interior-point step ends in the same kernel."""
    R, lay, P, bo, prm, GZ = _contact_start("go2", "whole_body_rnea", 4, nodes=20, batch=2, solver="fatrop")
    W = _wrench(2)
    bo.mpc_set_disturbance(base_wrench=W)
    try:
        seen = _run_contact(bo, R, lay, P, prm, GZ, W, 4, steps=2, lower_at=1, tag="fatrop")
    finally:
        bo.close()
    assert {"touchdown", "stick", "slide", "air"} <= seen, seen
