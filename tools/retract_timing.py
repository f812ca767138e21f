"""Time the batched device retract (pl_ocp_retract_device, k_retract.hip) at the headline shape.

Run on the GPU box:  python tools/retract_timing.py [--out FILE] [--commit ID] [robot dynamics N B]
(default b2g whole_body_rnea 50 1024, profiles/retract/retract_timing.json)

Measured on one handle after one solve, host clock around calls that end in a stream
synchronise (pl_ocp_retract_device returns after the kernel has finished):
  retract_device(steps=3) and retract_device(steps=N): median of 20 calls after 5 warm-ups;
  the `data` phase of pl_ocp_solve's phase_ms (values + Jacobian of every node: the all-node
  retract evaluates strictly less dynamics), median of 5 timed solves;
  the way to the same data without it: get_x() plus the host loop OCP.retract_stacked_sol over a
  sample of 8 problems, scaled to the batch (that loop returns no torques past tau_nodes and no
  equations-of-motion residual, so it does less per node).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "pino-locoman_amd"))
from pinoloco import _lib, robots  # noqa: E402
from pinoloco.ocp import OCP_ARGS, BatchedOCP, make_ocp  # noqa: E402
from pinoloco.synthetic import DT_MAX, DT_MIN, build_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retract", "retract_timing.json"))
ap.add_argument("--commit", default=None, help="recorded when the tree is not a git checkout")
ap.add_argument("shape", nargs="*", default=["b2g", "whole_body_rnea", "50", "1024"])
args = ap.parse_args()
rob, dyn, N, B = args.shape[0], args.shape[1], int(args.shape[2]), int(args.shape[3])
WARM, CALLS, SAMPLE = 5, 20, 8

import torch  # noqa: E402  (the device destination; fails without a GPU, there is no fallback)

R = robots.ROBOTS[rob]()
R.set_gait_sequence("trot", 0.8)
lay, P, X, XS, T0 = build_batch(R, dyn, N, B, 0)
bo = BatchedOCP(R, dyn, N, batch=B, device=0)
bo.set_params(P)
bo.set_x(X)
bo.init_solver()
bo.solve()
data_ms = float(np.median([bo.solve(timed=True)["phase_ms"][0] for _ in range(5)]))


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


res = {}
for steps in (3, N):
    total = bo.retract_sizes(steps)["total"]
    dst = torch.empty(total, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    res[f"retract_device_steps{steps}"] = dict(timed(lambda: bo.retract_device(dst.data_ptr(), steps)),
                                               doubles=total)

# the same data without the kernel: download x, retract problem by problem on the host
t0 = time.perf_counter()
Xs = bo.get_x()
get_x_ms = (time.perf_counter() - t0) * 1e3
ocp = make_ocp(dyn, OCP_ARGS[dyn], robot=R, nodes=N, solver="osqp")
ocp.set_time_params(DT_MIN, DT_MAX)
loop = []
for b in range(SAMPLE):
    ocp.update_initial_state(P[b, :lay.nx])
    t0 = time.perf_counter()
    ocp.retract_stacked_sol(Xs[b], True)
    loop.append((time.perf_counter() - t0) * 1e3)
host_ms = get_x_ms + float(np.mean(loop)) * B

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
out = {"shape": {"robot": rob, "dynamics": dyn, "N": N, "batch": B},
       "box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
       "commit": args.commit or commit or None, "lib_src_sha256": _lib.build_sha(),
       "calls": CALLS, "warmup": WARM,
       **res,
       "solve_data_phase_ms": data_ms,
       "host_loop": {"get_x_ms": get_x_ms, "per_problem_ms": float(np.mean(loop)), "sample": SAMPLE,
                     "scaled_to_batch_ms": host_ms}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
bo.close()
