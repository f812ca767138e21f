"""Generate the adaptive-rho fixtures tests/golden/adaptive_*.npz on the CPU.

The numpy oracle of the OCP (oracle/ocp.py) with its OSQP restatement replaced by the
adaptive-rho reference (tests/osqp_adaptive_ref.py), kkt="reduced_block" (the GPU's algebra);
the same solves with kkt="quasi_definite" give the stored CPU-to-CPU gap of dx.

Run from the repository root:  python tests/golden/make_golden_adaptive.py
Per fixture: B = 4 synthetic problems (the ("syn", k) problems of make_golden.py), one solve
each and, where `loop` > 0, a closed loop of that many MPC steps per problem.  The decision
log of every solve is stored as [K][4] rows (iteration, rho before, estimate, updated), NaN
padded.  The generator asserts what tests/test_adaptive_rho_gpu.py re-asserts from the log:
a problem with mid-solve updates, a problem without an update in its solve, an update at
it == max_iter that only the next solve of a loop sees, and no decision within 1 % of a
threshold.
"""
from __future__ import annotations

import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "pino-locoman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oracle.ocp import OracleOCP  # noqa: E402
from oracle.osqp_ref import REFERENCE_SETTINGS  # noqa: E402
from osqp_adaptive_ref import OSQPAdaptiveRef  # noqa: E402
from pinoloco import robots  # noqa: E402
from pinoloco.gait import horizon_dts  # noqa: E402
from pinoloco.ocp import Layout  # noqa: E402
from pinoloco.synthetic import DT_MAX, DT_MIN  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import make_problem  # noqa: E402

TOL = 5.0
KDEC = 4  # decisions per solve: max_iter 100 / interval 25
# name, robot, dynamics, N, synthetic problems, handle rho, closed-loop steps
CONFIGS = [
    ("adaptive_go2_rnea_n20", "go2", "whole_body_rnea", 20, [0, 1, 2, 3], 2e-2, 4),
    # at the handle rho of 2e-2 every synthetic problem updates at iteration 25 (no quiet problem
    # for the mask) and problem 3 takes a decision 0.97 % from a threshold; at 1e-2 problem 4 stays
    # inside the band for the whole solve beside three that update, all decisions >= 12 % away
    ("adaptive_go2_cv_n20", "go2", "centroidal_vel", 20, [0, 1, 2, 4], 1e-2, 0),
    # 2e-4 turns out to lie inside every problem's band (estimates 3e-4 .. 1e-3 < 5 x 2e-4): the
    # all-quiet fixture, with a problem that terminates at iteration 75.  No handle rho gives an
    # upward update at eps 1e-3 on these problems (at 2e-5 all four are solved by iteration 25,
    # before the first decision); tests/test_rho_adapt_host.py covers the upward branch of the rule.
    ("adaptive_go2_rnea_n20_rho2e-4", "go2", "whole_body_rnea", 20, [0, 1, 2, 3], 2e-4, 0),
]


def settings(rho):
    s = dict(REFERENCE_SETTINGS)
    s.update(rho=rho, adaptive_rho=True, adaptive_rho_interval=0, adaptive_rho_tolerance=TOL)
    return s


def adaptive_oracle(R, dyn, N, rho, kkt, x, p):
    o = OracleOCP(R, dyn, N, osqp_settings=settings(rho), kkt=kkt)
    o.init_solver(x, p)
    o.osqp = OSQPAdaptiveRef(o.hess_diag, o.pattern, o.osqp_settings, kkt=kkt, blocks=o.osqp.blocks)
    return o


def dec_array(decisions):
    a = np.full((KDEC, 4), np.nan)
    for k, d in enumerate(decisions):
        a[k] = [d[0], d[1], d[2], float(d[3])]
    return a


def _one(args):
    rname, dyn, N, gidx, rho, loop = args
    R = robots.ROBOTS[rname]()
    R.set_gait_sequence("trot", 0.8)
    lay = Layout(R, dyn, N)
    P0, X0, XS0, t0 = make_problem(R, lay, dyn, N, ("syn", gidx))
    out = dict(P=P0, X=X0, XS=XS0, T0=t0)
    for kkt in ("reduced_block", "quasi_definite"):
        o = adaptive_oracle(R, dyn, N, rho, kkt, X0, P0)
        x_new, dx, st = o.sqp_step(X0, P0)
        if kkt == "reduced_block":
            out.update(dx=dx, x_new=x_new, status=st["status"], iters=st["iter"], accepted=int(st["accepted"]),
                       branch=st["branch"], trials=st["trials"], alpha=st["alpha"], rho_b=o.osqp.rho_b,
                       dec=dec_array(o.osqp.decisions))
        else:
            out["dx_qd"] = dx
            out["dec_qd"] = dec_array(o.osqp.decisions)
    if loop:
        o = adaptive_oracle(R, dyn, N, rho, "reduced_block", X0, P0)
        xs, x = XS0.copy(), X0.copy()
        states, lst, decs, rhos = [], [], [], []
        for k in range(loop):
            p = P0.copy()
            contact, swing = R.gait_sequence.get_gait_schedule(t0 + k * DT_MIN, horizon_dts(DT_MIN, DT_MAX, N), N)
            vals = {"x_init": xs, "contact_schedule": contact, "swing_schedule": swing}
            for key in vals:
                o_, s_ = lay.poff[key]
                p[o_:o_ + s_] = lay.pack(vals)[o_:o_ + s_]
            if k > 0:
                x = o.warm_start(x, p)
            x, _, st = o.sqp_step(x, p)
            DX, _ = o.split(x)
            xs = o.integrate_state(xs, DX[1])
            states.append(xs)
            lst.append([st["status"], st["iter"], st["branch"], st["trials"]])
            decs.append(dec_array(o.osqp.decisions))
            rhos.append(o.osqp.rho_b)
        out.update(loop_states=np.array(states), loop_stats=np.array(lst), loop_dec=np.array(decs),
                   loop_rho_b=np.array(rhos))
    print(f"  {rname} {dyn} syn {gidx} rho {rho}: status {out['status']} iters {out['iters']} "
          f"updates at {[int(d[0]) for d in out['dec'] if d[3] == 1.0]} rho_b {out['rho_b']:.4g}", flush=True)
    return out


def margins(dec):
    """Smallest relative distance of a decision's estimate to either threshold."""
    d = dec.reshape(-1, 4)
    d = d[~np.isnan(d[:, 0])]
    if not len(d):
        return np.inf
    return float(min(np.min(np.abs(d[:, 2] / (d[:, 1] * TOL) - 1.0)), np.min(np.abs(d[:, 2] / (d[:, 1] / TOL) - 1.0))))


def properties(rec, max_iter=100):
    """What the fixture shows (the generator and the GPU test assert on these)."""
    dec = rec["dec"]
    mid = [(b, int(d[0])) for b in range(dec.shape[0]) for d in dec[b] if d[3] == 1.0 and d[0] < max_iter]
    none = [b for b in range(dec.shape[0]) if not np.any(dec[b][:, 3] == 1.0)]
    last = []  # (problem, step): an update at max_iter of a loop step that has a successor
    if "loop_dec" in rec:
        ld = rec["loop_dec"]
        for b in range(ld.shape[0]):
            for k in range(ld.shape[1] - 1):
                if any(d[3] == 1.0 and d[0] == max_iter for d in ld[b, k]):
                    assert ld[b, k + 1][0][1] == rec["loop_rho_b"][b, k]  # the next solve starts from it
                    last.append((b, k))
    m = min(margins(dec), margins(rec["loop_dec"]) if "loop_dec" in rec else np.inf)
    return dict(mid=mid, none=none, last=last, margin=m)


def fixture(name, rname, dyn, N, gidx, rho, loop):
    with ProcessPoolExecutor(min(len(gidx), int(os.environ.get("GOLDEN_WORKERS", "4")))) as ex:
        res = list(ex.map(_one, [(rname, dyn, N, g, rho, loop) for g in gidx]))
    rec = {"gidx": np.array(gidx), "gait": np.array("trot"), "rho": rho, "tolerance": TOL, "interval": 0,
           "osqp_max_iter": 100}
    for key in res[0]:
        rec[key] = np.array([r[key] for r in res])
    # CPU-to-CPU: the two formulations take the same decisions, and their steps differ by dx_gap
    assert np.array_equal(np.nan_to_num(rec["dec"][:, :, [0, 3]]), np.nan_to_num(rec["dec_qd"][:, :, [0, 3]])), name
    rec["dx_gap"] = np.array([np.abs(a - b).max() / np.abs(b).max() for a, b in zip(rec["dx"], rec["dx_qd"])])
    del rec["dx_qd"], rec["dec_qd"]
    pr = properties(rec)
    print(name, "status", rec["status"], "iters", rec["iters"], "dx gap", rec["dx_gap"], pr, flush=True)
    assert pr["margin"] > 0.01, (name, pr)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    return pr


def main():
    only = sys.argv[1:]
    prs = {c[0]: fixture(*c) for c in CONFIGS if not only or c[0] in only}
    if only:
        return
    assert any(pr["mid"] for pr in prs.values()), "no mid-solve update"
    assert any(pr["mid"] and pr["none"] for pr in prs.values()), "no fixture with an updating and a quiet problem"
    assert any(pr["last"] for pr in prs.values()), "no update at max_iter inside a loop"


if __name__ == "__main__":
    main()
