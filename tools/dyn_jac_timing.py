"""Time the batched point-function Jacobians (pl_dyn_jac_device, k_dyn_jac.hip) on B2G.

Run on the GPU box:  python tools/dyn_jac_timing.py [--out FILE] [--commit ID] [--batch B]
(default B = 4096, profiles/dyn_jac/dyn_jac_timing.json)

For the rnea, aba and frame_vel Jacobians with respect to every input:
  jac_device   pl_dyn_jac_device on torch tensors, bracketed by HIP events on the caller's stream
               and by the host clock (the call returns after the kernel has finished, so both
               include the launch and the stream synchronise): median, min, max of 20 calls after
               5 warm-ups;
  central_fd   the only route without it: 2 W central-difference calls of pl_dyn_eval on a device
               handle for the same points (host pointers: every call stages its inputs and its
               result over PCIe, which the device-pointer call avoids).  The perturbed inputs are
               built before the clock starts; the time is the 2 W evaluations alone, median of 3.
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
from pinoloco.dynamics import DynamicsWholeBodyTorque  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dyn_jac", "dyn_jac_timing.json"))
ap.add_argument("--commit", default=None, help="recorded when the tree is not a git checkout")
ap.add_argument("--batch", type=int, default=4096)
args = ap.parse_args()
B, WARM, CALLS, FD_REPS, EPS = args.batch, 5, 20, 3, 1e-6

import torch  # noqa: E402  (the device buffers; fails without a GPU, there is no fallback)

R = robots.ROBOTS["b2g"]()
R.set_gait_sequence("trot", 0.8)
rng = np.random.default_rng(3)
q = np.tile(R.q0, (B, 1))
q[:, 7:] += rng.normal(0, 0.2, (B, R.nj))
v, a = rng.normal(0, 0.5, (B, R.nv)), rng.normal(0, 1.0, (B, R.nv))
f = rng.normal(0, 50, (B, R.nf))
dev, host = DynamicsWholeBodyTorque(R, device=0), DynamicsWholeBodyTorque(R, device=-1)
ext = R.ext_force_frame
CASES = {"rnea": (dev.rnea_dynamics(ext), [q, v, a, f]),
         "aba": (dev.aba_dynamics(ext), [q, v, a[:, 6:], f]),
         "frame_vel": (dev.get_frame_velocity(R.foot_frames[0]), [q, v])}
integ = host.state_integrate()


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


res = {}
for name, (pf, ins) in CASES.items():
    tan, rows = pf.jacobian_sizes()
    W = sum(tan)
    tin = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ins]
    jac = torch.empty(B * rows * W, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ev, clk = [], []
    for it in range(WARM + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        pf.jacobian_device(B, [t.data_ptr() for t in tin], jac.data_ptr())
        e1.record()
        e1.synchronize()
        if it >= WARM:
            clk.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    # central differences through pl_dyn_eval: 2 W perturbed argument lists (q through integrate)
    pert = []
    for k, x in enumerate(ins):
        for c in range(tan[k]):
            for s in (EPS, -EPS):
                y = list(ins)
                if k == 0:
                    dx = np.zeros((B, 2 * R.nv))
                    dx[:, c] = s
                    y[0] = np.ascontiguousarray(integ(np.hstack([q, v]), dx)[:, :R.nq])
                else:
                    y[k] = x.copy()
                    y[k][:, c] += s
                pert.append(y)
    assert len(pert) == 2 * W
    pf(*ins)
    fd = []
    for _ in range(FD_REPS):
        t0 = time.perf_counter()
        for y in pert:
            pf(*y)
        fd.append((time.perf_counter() - t0) * 1e3)
    res[name] = {"W": W, "rows": rows, "jac_device_events": stats(ev), "jac_device_host_clock": stats(clk),
                 "central_fd_2W_evals": dict(stats(fd), evals=2 * W),
                 "ratio_fd_over_jac": float(np.median(fd) / np.median(ev))}

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
out = {"shape": {"robot": "b2g", "batch": B},
       "box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
       "commit": args.commit or commit or None, "lib_src_sha256": _lib.build_sha(), "calls": CALLS, "warmup": WARM,
       "note": "central_fd stages inputs and results over PCIe in every pl_dyn_eval call; jac_device does not",
       **res}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    json.dump(out, fo, indent=1)
print(json.dumps(out))
