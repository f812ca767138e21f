"""Ground contact and joint PD of the MPC plant (pl_mpc_set_contact / pl_mpc_get_contact /
pl_mpc_plant_host, include/pinoloco.h, csrc/plant.h) on host-only handles.

pl_mpc_plant_host runs the pl::plant_step the kernel runs, so the model is checked here without
a device against the numpy twin of tests/contact_ref.py, whose commands (tau_cmd, f_cmd, q_des,
v_des) are read from the iterate and x_init through Layout offsets, not from the code under test.

Bars (contact_ref.bars), all from the project's own: state 1e-10 x max(1, max |a|) (the ABA bar of
tests/test_plant_gpu.py); ground forces (k_n + k_t + d_n + d_t) x 1e-12 (the q / v bar through the
linear force law); anchors 1e-12 x (2 + d_t / k_t).  Every branch decision of the twin has to be
clear of round-off by 1e-9 and each of the five events has to occur, or the comparison shows
nothing."""
import numpy as np
import pytest

import contact_ref as cr
from conftest import make_robot

N, B = 6, 3
VARIANTS = [("go2", "whole_body_rnea"), ("b2g", "whole_body_rnea"), ("go2", "whole_body_aba")]


def _host(rname="go2", dyn="whole_body_rnea", batch=B, **kw):
    from pinoloco.ocp import BatchedOCP
    return BatchedOCP(make_robot(rname), dyn, N, batch=batch, device=-1, **kw)


def _problems(R, dyn, seed=3):
    """Synthetic problems 0..2, each with its own dt_min; the iterate is the initial guess plus a
    seeded perturbation."""
    from pinoloco.synthetic import DT_MIN, build_batch
    lay, P, X, XS, _ = build_batch(R, dyn, N, B, 0)
    P = P.copy()
    P[:, lay.poff["dt_min"][0]] = DT_MIN * (1.0 + 0.1 * np.arange(B))
    X = X + np.random.default_rng(seed).normal(size=X.shape) * 0.02
    return lay, P, X, XS


def _wrench(seed=5):
    return np.random.default_rng(seed).normal(size=(B, 6)) * np.array([20.0, 20.0, 20.0, 3.0, 3.0, 3.0])


def _ext(R):
    return R.ext_force_frame


def _frames(R):
    return list(R.foot_frames) + ([R.ext_force_frame] if R.ext_force_frame is not None else [])


# ---------------------------------------------------------------- settings, refusals
def test_contact_defaults_and_ground_under_feet():
    from oracle import rbd
    from pinoloco.ocp import contact_defaults
    bo = _host()
    R = bo.robot
    c = bo.contact_defaults()
    m = R.mass
    assert c["k_n"] == pytest.approx(m * 9.81 / (4 * 0.005), rel=1e-14)
    assert c["d_n"] == pytest.approx(2 * 0.3 * np.sqrt(c["k_n"] * m / 4), rel=1e-14)
    assert c["k_t"] == c["k_n"] and c["d_t"] == c["d_n"] and c["mu"] == 0.7 and c["kp"] == 0.0 and c["kd"] == 0.0
    c2 = bo.contact_defaults(penetration=0.01, zeta=0.1, mu=0.4, kp=40, kd=1)
    assert c2["k_n"] == pytest.approx(c["k_n"] / 2) and c2["mu"] == 0.4 and (c2["kp"], c2["kd"]) == (40.0, 1.0)
    assert contact_defaults(R) == c
    slick = _host(batch=1, mu=0.3)
    assert slick.contact_defaults()["mu"] == 0.3  # the OCP description's own coefficient
    slick.close()
    _, _, _, XS = _problems(R, "whole_body_rnea")
    gz = bo.ground_under_feet(XS, 0.005)
    M = rbd.ModelArrays(R.model)
    assert gz.shape == (B, 4)
    for b in range(B):
        _, oM = rbd.forward_kinematics(M, XS[b, :R.nq])
        for e, fid in enumerate(R.foot_frames):
            assert abs(gz[b, e] - (rbd.frame_placement(M, oM, fid)[1][2] + 0.005)) < 1e-12
    assert np.array_equal(bo.ground_under_feet(XS[0], 0.005), np.tile(gz[0], (B, 1)))  # one state for all
    assert np.array_equal(bo.ground_under_feet(R.q0), bo.ground_under_feet(np.concatenate([R.q0, np.zeros(R.nv)])))
    bo.close()


def test_set_and_get_need_a_device():
    from pinoloco import _lib
    bo = _host()
    c = bo.contact_defaults()
    with pytest.raises(_lib.PinolocoError, match="device"):
        bo.mpc_set_contact(c, np.zeros((B, 4)))
    with pytest.raises(_lib.PinolocoError, match="device"):
        bo.mpc_set_contact()
    with pytest.raises(_lib.PinolocoError, match="device"):
        bo.mpc_get_contact()
    assert _lib.lib().pl_mpc_set_contact(None, None, None) < 0
    # contact is a modifier of the "aba" plant, not a mode: the plant setting is untouched
    bo.mpc_set_plant("aba", 16)
    assert bo.mpc_get_plant() == ("aba", 16)
    bo.close()


def test_bad_contact_arguments_are_errors():
    from pinoloco import _lib
    bo = _host()
    R = bo.robot
    lay, P, X, XS = _problems(R, "whole_body_rnea")
    good = bo.contact_defaults(kp=40, kd=1)
    gz = np.zeros((B, 4))
    for name in cr.FIELDS:
        for bad in (-1.0, np.nan, np.inf):
            c = dict(good)
            c[name] = np.array([good[name], bad, good[name]])  # the refusal names the problem's field
            with pytest.raises(_lib.PinolocoError, match=name):
                bo.mpc_set_contact(c, gz)
            with pytest.raises(_lib.PinolocoError, match=name):
                bo.mpc_plant_host(P[0], X[0], XS[0], params=dict(good, **{name: bad}), ground_z=gz[0])
    with pytest.raises(_lib.PinolocoError, match="k_n"):
        bo.mpc_set_contact(dict(good, k_n=0.0), gz)
    with pytest.raises(_lib.PinolocoError, match="k_n"):
        bo.mpc_plant_host(P[0], X[0], XS[0], params=dict(good, k_n=0.0), ground_z=gz[0])
    # shapes, as mpc_set_disturbance
    for g in (np.zeros((B, 3)), np.zeros((B + 1, 4)), np.zeros(4), None):
        with pytest.raises(_lib.PinolocoError, match="ground_z"):
            bo.mpc_set_contact(good, g)
    for v in (np.zeros(B + 1), np.zeros((B, 1))):
        with pytest.raises(_lib.PinolocoError, match="mu"):
            bo.mpc_set_contact(dict(good, mu=v), gz)
    with pytest.raises(_lib.PinolocoError, match="missing"):
        bo.mpc_set_contact({k: good[k] for k in cr.FIELDS[:-1]}, gz)
    with pytest.raises(_lib.PinolocoError, match="unknown"):
        bo.mpc_set_contact(dict(good, k_x=1.0), gz)
    for sub in (0, 17):
        with pytest.raises(_lib.PinolocoError, match="substeps"):
            bo.mpc_plant_host(P[0], X[0], XS[0], substeps=sub)
    with pytest.raises(_lib.PinolocoError, match="x_state"):
        bo.mpc_plant_host(P[0], X[0], XS[0][:-1])
    with pytest.raises(_lib.PinolocoError, match="anchors"):
        bo.mpc_plant_host(P[0], X[0], XS[0], params=good, ground_z=gz[0], anchors=np.zeros((3, 3)))
    with pytest.raises(_lib.PinolocoError, match="ground_z"):
        bo.mpc_plant_host(P[0], X[0], XS[0], params=good)
    bo.close()


@pytest.mark.parametrize("include_base", [True, False])
def test_contact_refused_on_centroidal_vel(include_base):
    from pinoloco import _lib
    bo = _host(dyn="centroidal_vel", include_base=include_base)
    c = bo.contact_defaults()
    with pytest.raises(_lib.PinolocoError, match="centroidal_vel"):
        bo.mpc_set_contact(c, np.zeros((B, 4)))
    with pytest.raises(_lib.PinolocoError, match="centroidal_vel"):
        bo.mpc_plant_host(np.zeros(bo.np), np.zeros(bo.n), np.zeros(bo.layout.nx), params=c, ground_z=np.zeros(4))
    bo.close()


# ---------------------------------------------------------------- the model against the twin
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("rname,dyn", VARIANTS, ids=[f"{r}-{d}" for r, d in VARIANTS])
def test_plant_host_matches_twin(rname, dyn, substeps):
    """Three calls per problem, each teacher-forced from the host's own previous output: the
    inputs of contact_ref.case_inputs (air, stick and slide at the first substep, touchdown of
    every foot in contact), then the ground under one contacting foot lowered by 2 cm (lift-off),
    then raised again (touchdown with a fresh anchor)."""
    from oracle import rbd
    bo = _host(rname, dyn)
    R = bo.robot
    M = rbd.ModelArrays(R.model)
    lay, P, X, XS = _problems(R, dyn)
    W = _wrench()
    prm, GZ = cr.case_inputs(bo, XS)
    seen, worst, first = set(), {"x": 0.0, "f": 0.0, "anchor": 0.0}, []
    o = lay.poff["x_init"][0]
    for b in range(B):
        c = cr.one(prm, b)
        tau, f, qd, vd = cr.commands(lay, X[b], P[b, o:o + lay.nx])
        dt_min = P[b, lay.poff["dt_min"][0]]
        xs, anc = XS[b].copy(), np.zeros((4, 3))
        foot = None
        for call in range(3):
            gz = GZ[b].copy()
            if call == 1 and anc[:, 2].any():  # a foot that stands by now (the substeps may have thrown some off)
                foot = int(np.argmax(anc[:, 2]))
                old_anchor = anc[foot].copy()
            if call == 1 and foot is not None:
                gz[foot] -= 0.02
            if call == 2 and foot is not None:  # raised again, to 4 mm above where the foot is by now
                gz[foot] = bo.ground_under_feet(xs, 0.004)[b, foot]
            got = bo.mpc_plant_host(P[b], X[b], xs, substeps, W[b], c, gz, anc)
            want = cr.contact_plant(M, R.foot_frames, _ext(R), R.nq, xs, tau, f, qd, vd, W[b], dt_min, substeps, c,
                                    gz, anc)
            cr.check_log(want[4], seen)
            ev = {(s, e): v for s, e, v, _, _ in want[4]}
            if call == 0:
                first.append([ev[0, e] for e in range(4)])
            if call == 1 and foot is not None:
                assert "liftoff" in ev[0, foot] and got[1][foot, 2] == 0.0, (b, ev)
            if call == 2 and foot is not None:
                assert "touchdown" in ev[0, foot], (b, ev)
                assert not np.array_equal(want[1][foot, :2], old_anchor[:2])  # a fresh anchor
            bx, bf, ba = cr.bars(c, want[3])
            ex, ea, ef = (np.abs(got[k] - want[k]).max() for k in range(3))  # state, anchors, forces
            worst = {"x": max(worst["x"], ex / bx), "f": max(worst["f"], ef / bf), "anchor": max(worst["anchor"], ea / ba)}
            assert ex < bx and ef < bf and ea < ba, (b, call, (ex, bx), (ef, bf), (ea, ba))
            assert np.all(np.isfinite(got[0]))
            xs, anc = got[0], got[1]
    print("contact host", rname, dyn, f"substeps={substeps}", "worst error / bar",
          {k: f"{v:.2e}" for k, v in worst.items()}, "first substep", first)
    assert seen == set(cr.EVENTS), seen
    bo.close()


def test_contact_off_is_the_aba_plant():
    """prm = NULL is the numpy ABA plant of tests/test_plant_gpu.py.  A ground far below (-10 m)
    with kp = kd = 0 is that plant too, except that the feet's commanded forces are gone."""
    from oracle import rbd
    bo = _host("b2g", "whole_body_rnea")
    R = bo.robot
    M = rbd.ModelArrays(R.model)
    lay, P, X, XS = _problems(R, "whole_body_rnea")
    W = _wrench()
    o = lay.poff["x_init"][0]
    c = bo.contact_defaults()
    for b in range(B):
        tau, f, qd, vd = cr.commands(lay, X[b], P[b, o:o + lay.nx])
        dt_min = P[b, lay.poff["dt_min"][0]]
        anc0 = np.random.default_rng(b).normal(size=(4, 3))
        got, anc, forces = bo.mpc_plant_host(P[b], X[b], XS[b], 4, W[b], anchors=anc0)
        want, amax = cr.aba_plant(M, _frames(R), R.nq, XS[b], tau, f, W[b], dt_min, 4)
        assert np.abs(got - want).max() < 1e-10 * max(1.0, amax), b
        assert np.array_equal(anc, anc0) and not forces.any()  # not touched without contact
        low = np.full(4, -10.0)
        got, anc, forces = bo.mpc_plant_host(P[b], X[b], XS[b], 4, W[b], c, low, np.zeros((4, 3)))
        twin = cr.contact_plant(M, R.foot_frames, _ext(R), R.nq, XS[b], tau, f, qd, vd, W[b], dt_min, 4, c, low,
                                np.zeros((4, 3)))
        f0 = f.copy()
        f0[:12] = 0.0
        assert f0[12:].any()  # B2G: the external-force frame keeps its command
        plain, amax = cr.aba_plant(M, _frames(R), R.nq, XS[b], tau, f0, W[b], dt_min, 4)
        tol = 1e-10 * max(1.0, amax)
        assert np.abs(got - twin[0]).max() < tol and np.abs(got - plain).max() < tol, b
        assert not anc.any() and not forces.any()
    bo.close()


def test_standing_on_the_ground():
    """Go2 at q0 with the static RNEA torques as feed-forward, PD (40, 1), the default ground 5 mm
    under the feet, 16 substeps, 60 steps: the base stays within one nominal penetration (5 mm) of
    its start, |v| < 0.05 and all four feet stick.  (A numpy prototype of the model gave 0.9 mm
    and 1.3e-3.)"""
    from oracle import rbd
    from pinoloco.synthetic import problem_values
    bo = _host(batch=1)
    R = bo.robot
    M = rbd.ModelArrays(R.model)
    lay = bo.layout
    x0 = np.concatenate([R.q0, np.zeros(R.nv)])
    vals, _, _ = problem_values(R, "whole_body_rnea", N, 0, lay)
    vals["x_init"] = x0
    p = lay.pack(vals)
    fz = np.tile([0.0, 0.0, R.mass * 9.81 / 4], 4)
    tau = rbd.rnea_dynamics(M, list(R.foot_frames), R.q0, np.zeros(R.nv), np.zeros(R.nv), fz)[6:]
    x = np.zeros(lay.n)
    u0 = lay.x_off[0] + lay.ndx
    x[u0 + lay.tau_idx:u0 + lay.tau_idx + lay.nj] = tau
    c = bo.contact_defaults(kp=40, kd=1)
    gz = bo.ground_under_feet(R.q0, 0.005)[0]
    xs, anc = x0.copy(), None
    for _ in range(60):
        xs, anc, forces = bo.mpc_plant_host(p, x, xs, 16, None, c, gz, anc)
    drift, vmax = np.abs(xs[:3] - x0[:3]).max(), np.abs(xs[R.nq:]).max()
    ft = np.hypot(forces[:, 0], forces[:, 1])
    print("standing: base drift", f"{drift:.2e}", "max |v|", f"{vmax:.2e}", "ft / (mu fn)", ft / (c["mu"] * forces[:, 2]))
    assert np.all(np.isfinite(xs))
    assert drift < 0.005 and vmax < 0.05, (drift, vmax)
    assert np.all(anc[:, 2] == 1.0) and np.all(forces[:, 2] > 0) and np.all(ft < c["mu"] * forces[:, 2]), forces
    bo.close()
