"""In-process A/B of k_admm's operand paths (pl_ocp_set_admm_operands) at the headline config.

Run on the GPU box:  python tools/gpu_admm_operands_ab.py [steps] [B]

One handle runs the benchmark's MPC loop (B2G whole_body_rnea, N = 50) with the per-launch
events on (eager launches); step k uses "split" when k is even and "fused" when odd.  The two
paths give the same bits, so the loop's trajectory does not depend on the alternation, and
neighbouring steps see the same box state: the ratio is free of the drift between processes
that the bench.py A/B of two libraries carries.  Prints ms per launch and ns per
problem-iteration of each step, then the medians and the median of the paired ratios.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pino-locoman_amd"))
from pinoloco import robots  # noqa: E402
from pinoloco.ocp import BatchedOCP  # noqa: E402
from pinoloco.synthetic import build_batch  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
N = 50
R = robots.ROBOTS["b2g"]()
R.set_gait_sequence("trot", 0.8)
lay, P, X, XS, T0 = build_batch(R, "whole_body_rnea", N, B, 0)
bo = BatchedOCP(R, "whole_body_rnea", N, batch=B, device=0)
bo.set_admm_kernel("sweep")
bo.set_params(P)
bo.set_x(X)
bo.init_solver()
bo.mpc_setup(XS, T0)
for k in range(2):  # warm-up, one step per mode
    bo.set_admm_operands(("split", "fused")[k])
    bo.mpc_step(k)
bo.sync()
res = {"split": [], "fused": []}
for k in range(2, 2 + steps):
    mode = ("split", "fused")[k % 2]
    bo.set_admm_operands(mode)
    bo.profile(1)
    bo.mpc_step(k)
    bo.sync()
    pr = bo.profile_read()
    bo.profile(0)
    ms, ns = pr["admm_ms"] / pr["launches"], 1e6 * pr["admm_ms"] / pr["problem_iters"]
    res[mode].append((ms, ns))
    print(f"step {k:3d} {mode:5s} launches {pr['launches']} ms/launch {ms:8.3f} ns/problem-iter {ns:8.2f}")
s, f = np.array(res["split"]), np.array(res["fused"])
n = min(len(s), len(f))
for name, a in (("split", s), ("fused", f)):
    print(f"{name}: median ms/launch {np.median(a[:, 0]):.3f}  median ns/problem-iter {np.median(a[:, 1]):.2f}  "
          f"min {a[:, 1].min():.2f} max {a[:, 1].max():.2f}")
ratio = f[:n, 1] / s[:n, 1]
print(f"fused / split, ns per problem-iter, paired neighbours: median {np.median(ratio):.4f}  "
      f"min {ratio.min():.4f} max {ratio.max():.4f}  ({n} pairs)")
bo.close()
