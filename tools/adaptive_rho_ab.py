"""A/B of OSQP's adaptive rho at the headline shape (B2G whole_body_rnea, N = 50, batch 1024,
build_batch's problems, the device MPC loop as bench.py drives it).

Three runs, each in a process of its own under its own time limit, back to back on one GPU:
  off     the default (rho from the bounds in the fused sweep): what the parent commit runs
  on      set_adaptive_rho(True): interval = check_termination, tolerance 5
  stream  set_adaptive_rho(True, tolerance=1e30): no estimate ever leaves the band, so the run
          pays for streaming d.rho, the scaled norms, k_rho_adapt and the empty masked
          dispatches, and takes no update
Per run: 5 warm-up steps and 20 timed steps (no host reads inside the timed region), then the
same 25 steps again from the same start with the per-step outcome read back.  Writes
profiles/adaptive_rho/ab.json (or --out).

  python tools/adaptive_rho_ab.py [--out FILE] [--steps 20] [--warmup 5] [--batch 1024]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "pino-locoman_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = {"off": None, "on": (True, 0, 5.0), "stream": (True, 0, 1e30)}


def _dist(v):
    import numpy as np
    v = np.asarray(v, dtype=float)
    f = v[np.isfinite(v)]
    q = (lambda p: float(np.quantile(f, p))) if f.size else (lambda p: None)
    return {"min": q(0.0), "p50": q(0.5), "p90": q(0.9), "max": q(1.0), "mean": float(f.mean()) if f.size else None,
            "nonfinite": int(v.size - f.size)}


def child(args):
    import numpy as np
    from pinoloco import robots
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    R = robots.ROBOTS[args.robot]()
    R.set_gait_sequence("trot", 0.8)
    lay, P, X, XS, T0 = build_batch(R, args.dynamics, args.nodes, args.batch, 0)
    bo = BatchedOCP(R, args.dynamics, args.nodes, batch=args.batch, device=0, gait_type="trot", gait_period=0.8)
    if MODES[args.mode]:
        bo.set_adaptive_rho(*MODES[args.mode])

    def start():
        bo.set_params(P)
        bo.set_x(X)
        bo.init_solver()
        bo.mpc_setup(XS, T0)

    start()
    for k in range(args.warmup):
        bo.mpc_step(k)
    bo.sync()
    t0 = time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        bo.mpc_step(k)
    bo.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    graph = bo.mpc_graph_info()
    start()
    iters, status, upd, viol, f = [], {}, [], [], []
    for k in range(args.warmup + args.steps):
        bo.mpc_step(k)
        if k < args.warmup:
            continue
        st = bo.mpc_stats()
        iters.append(float(np.mean(st["admm_iters"])))
        for s, c in zip(*np.unique(st["status"], return_counts=True)):
            status[int(s)] = status.get(int(s), 0) + int(c)
        upd.append(bo.osqp_rho()["updates"])
        viol.append(st["viol_max"])
        f.append(st["f"])
    upd = np.array(upd)  # [steps][B]
    per_problem = upd.mean(axis=0)  # updates per solve, per problem
    rho = bo.osqp_rho()["rho"]
    out = {"mode": args.mode, "ms_per_step": ms, "mean_admm_iters_per_solve": float(np.mean(iters)),
           "admm_iters_per_step": iters, "status_histogram": status,
           "rho_updates_per_solve": {"min": float(per_problem.min()), "median": float(np.median(per_problem)),
                                     "max": float(per_problem.max())},
           "viol_max": _dist(np.concatenate(viol)), "f": _dist(np.concatenate(f)), "rho_final": _dist(rho),
           "rho_from_bounds": bool(bo.admm_rho_from_bounds()), "admm_kernel": bo.admm_kernel(), "graph": graph,
           "finite_state": bool(np.all(np.isfinite(bo.mpc_state())))}
    bo.close()
    print("AB_RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_rho", "ab.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--robot", default="b2g")
    ap.add_argument("--dynamics", default="whole_body_rnea")
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per run")
    ap.add_argument("--mode", default=None, choices=sorted(MODES), help="(internal) one run in this process")
    args = ap.parse_args()
    if args.mode:
        child(args)
        return 0
    res = {"shape": {"robot": args.robot, "dynamics": args.dynamics, "nodes": args.nodes, "batch": args.batch,
                     "warmup": args.warmup, "steps": args.steps}, "runs": {}}
    for mode in ("off", "on", "stream"):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode] + [
            f"--{k}={getattr(args, k)}" for k in ("steps", "warmup", "batch", "robot", "dynamics", "nodes")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{mode}: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB_RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1  # nothing more on this GPU after a failed run
        res["runs"][mode] = json.loads(line[0][len("AB_RESULT "):])
        print(mode, json.dumps({k: res["runs"][mode][k] for k in ("ms_per_step", "mean_admm_iters_per_solve",
                                                                  "status_histogram", "rho_updates_per_solve")}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
