"""Shared by tests/test_dyn_jac_host.py and tests/test_dyn_jac_gpu.py: the supported point
functions of pl_dyn_jac as (name, PointFunction, arguments) cases, the test points, and the
complex-step reference Jacobian built from oracle/rbd.py (which accepts complex inputs).

Reference: column k of a configuration block is Im f(rbd.integrate(M, q + 0j, 1j h e_k)) / h with
h = 1e-30; Euclidean inputs are stepped directly.  The complex step has no subtraction, so the
reference is exact to round-off.
"""
import numpy as np

from conftest import golden, make_robot

H = 1e-30
ROBOTS = ("go2", "b2g")
# functions whose value goes through a linear solve (the 1e-10 class of tests/test_dynamics.py)
SOLVE = ("aba", "base_acc_wb", "base_vel_cv", "base_acc_cv")


def points(name):
    """The three points of tests/golden/rbd_<robot>.npz (generic base quaternion, w = 0.04) plus
    one with the base yawed 170 degrees about z and the joint angles offset by N(0, 0.2)."""
    G = golden(f"rbd_{name}.npz")
    R = make_robot(name)
    rng = np.random.default_rng(11)
    P = {k: np.array(G[k]) for k in ("q", "v", "a", "f", "h", "a_j", "v_j")}
    P["tau_j"] = np.array(G["tau"])[:, 6:]
    q = np.array(R.q0, dtype=float)
    half = np.deg2rad(170.0) / 2
    q[3:7] = [0.0, 0.0, np.sin(half), np.cos(half)]
    q[7:] += rng.normal(0, 0.2, R.nj)
    extra = dict(q=q, v=rng.normal(0, 0.5, R.nv), a=rng.normal(0, 1.0, R.nv), f=rng.normal(0, 50, P["f"].shape[1]),
                 h=rng.normal(0, 0.5, 6), tau_j=rng.normal(0, 10, R.nj))
    extra["a_j"], extra["v_j"] = extra["a"][6:], extra["v"][6:]
    return {k: np.vstack([P[k], extra[k][None]]) for k in P}, R, list(G["frames"])


def batch67(name):
    """67 points: the four above and perturbed copies."""
    P, R, frames = points(name)
    rng = np.random.default_rng(5)
    out = {}
    for k, a in P.items():
        rep = np.tile(a, (17, 1))[:67].copy()
        rep[4:] += rng.normal(0, 0.05, rep[4:].shape) * (1.0 if k != "f" else 20.0)
        out[k] = rep
    qn = out["q"][:, 3:7]
    out["q"][:, 3:7] = qn / np.linalg.norm(qn, axis=1, keepdims=True)
    out["a_j"], out["v_j"] = out["a"][:, 6:].copy(), out["v"][:, 6:].copy()
    return out, R, frames


def cases(name, device=-1):
    """[(case name, PointFunction, input keys, index of the configuration input)]."""
    from pinoloco.dynamics import (DynamicsCentroidalAcc, DynamicsCentroidalVel, DynamicsWholeBodyAcc,
                                   DynamicsWholeBodyTorque)
    R = make_robot(name)
    ext = R.ext_force_frame
    wb, acc = DynamicsWholeBodyTorque(R, device=device), DynamicsWholeBodyAcc(R, device=device)
    cv, ca = DynamicsCentroidalVel(R, device=device), DynamicsCentroidalAcc(R, device=device)
    foot = R.foot_frames[0]
    out = [("rnea", wb.rnea_dynamics(ext), ("q", "v", "a", "f"), 0),
           ("aba", wb.aba_dynamics(ext), ("q", "v", "tau_j", "f"), 0),
           ("nle", wb.nonlinear_effects(), ("q", "v"), 0),
           ("frame_pos", wb.get_frame_position(foot), ("q",), 0),
           ("frame_vel", wb.get_frame_velocity(foot), ("q", "v"), 0),
           ("gaps_wb", acc.dynamics_gaps(ext), ("q", "v", "a", "f"), 0),
           ("base_acc_wb", acc.base_acc_dynamics(ext), ("q", "v", "a_j", "f"), 0),
           ("com_dyn", cv.com_dynamics(ext), ("q", "f"), 0),
           ("base_vel_cv", cv.base_vel_dynamics(), ("h", "q", "v_j"), 1),
           ("base_acc_cv", cv.base_acc_dynamics(ext), ("q", "v", "a_j", "f"), 0),
           ("gaps_cv", cv.dynamics_gaps(), ("h", "q", "v"), 1),
           ("com", wb.center_of_mass(), ("q",), 0),
           ("gaps_ca", ca.dynamics_gaps(ext), ("q", "v", "a", "f"), 0)]
    if R.arm_ee_frame is not None:
        out.append(("frame_vel_rel", wb.get_frame_velocity(R.arm_ee_frame, relative_to_base=True), ("q", "v"), 0))
    return out, R


def oracle_fn(case, R, frames):
    """The oracle's value function of a case, on (possibly complex) arrays."""
    from oracle import rbd
    Mo = rbd.ModelArrays(R.model)
    m = R.mass
    foot = R.foot_frames[0]
    base = R.model.get_frame_id("base_link")
    return {
        "rnea": lambda q, v, a, f: rbd.rnea_dynamics(Mo, frames, q, v, a, f),
        "aba": lambda q, v, t, f: rbd.aba_dynamics(Mo, frames, q, v, t, f),
        "nle": lambda q, v: rbd.rnea(Mo, q, v, np.zeros_like(v)),
        "frame_pos": lambda q: rbd.frame_placement(Mo, rbd.forward_kinematics(Mo, q)[1], foot)[1],
        "frame_vel": lambda q, v: rbd.frame_velocity(Mo, q, v, foot),
        "frame_vel_rel": lambda q, v: rbd.frame_velocity(Mo, q, v, R.arm_ee_frame, True, base),
        "gaps_wb": lambda q, v, a, f: rbd.rnea_dynamics(Mo, frames, q, v, a, f)[..., :6],
        "base_acc_wb": lambda q, v, aj, f: rbd.base_acc_wb(Mo, frames, q, v, aj, f),
        "com_dyn": lambda q, f: rbd.com_dynamics(Mo, frames, q, f, m),
        "base_vel_cv": lambda h, q, vj: rbd.base_vel_cv(Mo, h, q, vj, m),
        # A_b^-1 (dh - dA v - A_j a_j) in its arithmetic-only form: rbd.base_acc_cv takes dA v from
        # a complex step of its own (dccrba_v), which an outer complex step cannot pass through
        "base_acc_cv": lambda q, v, aj, f: rbd.base_acc_ca(Mo, frames, q, v, aj, f, m),
        "gaps_cv": lambda h, q, v: rbd.centroidal_momentum(Mo, q, v) - m * h,
        "com": lambda q: rbd.center_of_mass(Mo, q),
        "gaps_ca": lambda q, v, a, f: rbd.gaps_ca(Mo, frames, q, v, a, f, m),
    }[case], Mo


def complex_step_blocks(fun, Mo, args, cfg):
    """One block per input of fun(*args) at a single point; input `cfg` is a configuration.
    All columns of a block go through the oracle in one call (its functions take leading batch
    dimensions)."""
    from oracle import rbd
    blocks = []
    for k, x in enumerate(args):
        n = Mo.nv if k == cfg else len(x)
        E = 1j * H * np.eye(n)
        xs = [np.tile(np.asarray(a, dtype=complex), (n, 1)) for a in args]
        xs[k] = rbd.integrate(Mo, xs[k], E) if k == cfg else xs[k] + E
        blocks.append(np.imag(fun(*xs)).T / H)
    return blocks
