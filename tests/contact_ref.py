"""Numpy twin of the contact plant (include/pinoloco.h pl_mpc_set_contact, csrc/plant.h), from the
oracle's own pieces: rbd.joint_velocities, frame_placement and frame_velocity_lwa for the foot's
position and LOCAL_WORLD_ALIGNED velocity, rbd.contact_fext and rbd.aba for the forward dynamics,
rbd.integrate for the state map, in the shape of tests/test_plant_gpu.py::_numpy_plant.

Per substep and foot it also reports the branch taken and how far the inputs were from the
branch conditions, so that a test can require that no decision hangs on round-off:
  events   a tuple out of "air", "liftoff" (in the air with an anchor still active), "touchdown"
           (in contact without one), "stick", "slide"
  d        |ground_z - p.z|, the distance from the contact switch
  cone     |nrm - lim| / max(lim, tiny) in contact (inf in the air)
"""
import numpy as np

from oracle import rbd

TINY = 1e-300
EVENTS = ("air", "liftoff", "touchdown", "stick", "slide")
FIELDS = ("k_n", "d_n", "k_t", "d_t", "mu", "kp", "kd")


def ground_force(c, gz, p, u, anchor):
    """The model's force on one foot; anchor (x, y, active) is updated in place."""
    d = gz - p[2]
    if not d > 0:
        ev = ("air", "liftoff") if anchor[2] else ("air",)
        anchor[2] = 0.0
        return np.zeros(3), ev, abs(d), np.inf
    ev = ()
    fn = max(0.0, c["k_n"] * d - c["d_n"] * u[2])
    if not anchor[2]:
        anchor[:] = (p[0], p[1], 1.0)
        ev += ("touchdown",)
    ft = -c["k_t"] * (p[:2] - anchor[:2]) - c["d_t"] * u[:2]
    lim = c["mu"] * fn
    nrm = np.sqrt(ft[0] ** 2 + ft[1] ** 2)
    if nrm > lim:
        ft = ft * (lim / nrm)
        if c["k_t"] > 0:
            anchor[:2] = p[:2] + (ft + c["d_t"] * u[:2]) / c["k_t"]
        ev += ("slide",)
    else:
        ev += ("stick",)
    return np.array([ft[0], ft[1], fn]), ev, abs(d), abs(nrm - lim) / max(lim, TINY)


def foot_states(M, feet, q, v):
    """World position and LOCAL_WORLD_ALIGNED linear velocity of every foot frame."""
    _, oM, vs = rbd.joint_velocities(M, q, v)
    return oM, [(rbd.frame_placement(M, oM, fid)[1], rbd.frame_velocity_lwa(M, oM, vs, fid)[:3]) for fid in feet]


def contact_plant(M, feet, ext, nq, xs, tau_cmd, f_cmd, q_des, v_des, w, dt_min, substeps, c, ground_z, anchors):
    """substeps x { f = ground(feet) | f_cmd(ext); tau = tau_cmd + kp (q_des - q_j) + kd (v_des - v_j);
    a = ABA(q, v, [w; tau], f); q <- integrate(q, v h); v <- v + a h }.
    c: dict of FIELDS; q_des, v_des: joint parts [nj]; f_cmd [3 nee] (read for the ext frame only);
    anchors [n_feet][3].  Returns (state, anchors, forces of the last substep [n_feet][3], max |a|, log),
    log = [(substep, foot, events, d margin, cone margin)]."""
    q, v = xs[:nq].copy(), xs[nq:].copy()
    anchors = np.array(anchors, dtype=float)
    frames = list(feet) + ([ext] if ext is not None else [])
    h = dt_min / substeps
    amax, log = 0.0, []
    forces = np.zeros((len(feet), 3))
    for s in range(substeps):
        oM, fs = foot_states(M, feet, q, v)
        f = np.array(f_cmd, dtype=float).copy()
        for e, (p, u) in enumerate(fs):
            forces[e], ev, md, mc = ground_force(c, ground_z[e], p, u, anchors[e])
            f[3 * e:3 * e + 3] = forces[e]
            log.append((s, e, ev, md, mc))
        tau = tau_cmd + c["kp"] * (q_des - q[7:]) + c["kd"] * (v_des - v[6:])
        a = rbd.aba(M, q, v, np.concatenate([w, tau]), rbd.contact_fext(M, oM, frames, f))
        amax = max(amax, np.abs(a).max())
        q = rbd.integrate(M, q, v * h)
        v = v + a * h
    return np.concatenate([q, v]), anchors, forces, amax, log


def aba_plant(M, frames, nq, xs, tau, f, w, dt_min, substeps):
    """The plant without contact, the composition of tests/test_plant_gpu.py::_numpy_plant:
    substeps x { a = ABA(q, v, [w; tau], f); q <- integrate(q, v h); v <- v + a h }; also max |a|."""
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


def bars(c, amax):
    """(state, force, anchor) bars of the contact tests, all from the project's own: the ABA bar
    1e-10 x max(1, max |a|) for the state; the q / v bar 1e-12 through the linear force law,
    (k_n + k_t + d_n + d_t) x 1e-12; the anchors 1e-12 x (2 + d_t / k_t)."""
    return (1e-10 * max(1.0, amax), (c["k_n"] + c["k_t"] + c["d_n"] + c["d_t"]) * 1e-12,
            1e-12 * (2.0 + c["d_t"] / c["k_t"]))


GROUND_MM = (4.0, 1.0, -3.0, 6.0)   # ground above each foot frame, rolled by the problem index
MU = (0.7, 0.02, 1.0)
GAINS = ((40.0, 1.0), (0.0, 0.0), (10.0, 0.5))   # (kp, kd) per problem


def case_inputs(bo, xs):
    """The contact tests' inputs for a batch of up to three states: the default stiffnesses at
    5 mm and zeta = 0.3, per-problem mu and PD gains, and a ground that gives air, stick and slide
    at the first substep.  Returns (params: dict of [batch] arrays, ground_z [batch][n_feet])."""
    B = len(xs)
    c = bo.contact_defaults(penetration=0.005, zeta=0.3)
    prm = {k: np.full(B, c[k]) for k in FIELDS}
    prm["mu"] = np.array(MU[:B])
    prm["kp"] = np.array([g[0] for g in GAINS[:B]])
    prm["kd"] = np.array([g[1] for g in GAINS[:B]])
    gz = bo.ground_under_feet(xs, 0.0) + np.stack([np.roll(GROUND_MM, b) for b in range(B)]) * 1e-3
    return prm, gz


def one(prm, b):
    return {k: float(prm[k][b]) for k in FIELDS}


def check_log(log, seen):
    """Every branch decision of a twin run clear of round-off (1e-9); the events into `seen`."""
    for s, e, ev, md, mc in log:
        seen.update(ev)
        assert md > 1e-9 and mc > 1e-9, (s, e, ev, md, mc)


def commands(lay, x, x_init):
    """tau_cmd, f_cmd of node 0 and the joint q_des, v_des of node 1, read from the iterate and
    x_init through Layout offsets (whole_body_rnea with tau at node 0, whole_body_aba)."""
    u = x[lay.x_off[0] + lay.ndx:lay.x_off[0] + lay.ndx + lay.nu[0]]
    if lay.dynamics == "whole_body_aba":
        tau = u[:lay.nj]
    else:
        assert lay.dynamics == "whole_body_rnea" and lay.tau_nodes > 0
        tau = u[lay.tau_idx:lay.tau_idx + lay.nj]
    f = u[lay.f_idx:lay.f_idx + lay.nf]
    dx1 = x[lay.x_off[1]:lay.x_off[1] + lay.ndx]
    q_des = x_init[7:lay.nq] + dx1[6:lay.nv]
    v_des = x_init[lay.nq + 6:] + dx1[lay.nv + 6:]
    return tau.copy(), f.copy(), q_des, v_des
