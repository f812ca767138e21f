"""Demo of the gait and command timelines: stand -> trot -> walk with a velocity ramp, on the contact plant.

Go2 whole_body_rnea, N = 20, B = 8, 150 MPC steps (1.5 s) from the standing pose, "aba" plant with 16
substeps, contact_defaults with PD (kp 40, kd 1), the ground 5 mm under the standing feet.  Every
problem stands until step 30, trots from 30 while its forward velocity command ramps from 0 to its
own target (0 ... --vx-max across the batch) at step 80, holds it, and walks from step 110 at half
that speed.  The whole rollout runs on the device: mpc_set_timeline + mpc_log_start + mpc_run; the
host reads the metrics and the log once at the end.

Prints per problem: the velocity target, whether the state stayed finite, the largest height
deviation, the smallest tilt cosine, the steps not solved, and the base's forward speed at the end
of each phase.  Nothing here is a pass bar and nothing is tuned to it: it records what the loop
does.  --json writes the same to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "pino-locoman_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--nodes", type=int, default=20)
ap.add_argument("--substeps", type=int, default=16)
ap.add_argument("--kp", type=float, default=40.0)
ap.add_argument("--kd", type=float, default=1.0)
ap.add_argument("--vx-max", type=float, default=0.4)
ap.add_argument("--json", default=None)
a = ap.parse_args()

from pinoloco import robots  # noqa: E402
from pinoloco.ocp import BatchedOCP  # noqa: E402
from pinoloco.synthetic import initial_guess, problem_values  # noqa: E402

K_TROT, K_FULL, K_WALK, STEPS = 30, 80, 110, 150
B, N = a.batch, a.nodes
R = robots.ROBOTS["go2"]()
R.set_gait_sequence("stand", 0.5)
bo = BatchedOCP(R, "whole_body_rnea", N, batch=B, device=0, gait_type="stand", gait_period=0.5)
lay = bo.layout
vals, _, _ = problem_values(R, "whole_body_rnea", N, 0, lay)
x0 = np.concatenate([R.q0, np.zeros(R.nv)])
vals["x_init"] = x0
bo.set_params(np.tile(lay.pack(vals), (B, 1)))
bo.set_x(np.tile(initial_guess(R, lay, vals["n_contacts"]), (B, 1)))
bo.init_solver()
bo.mpc_setup(np.tile(x0, (B, 1)), np.zeros(B))
bo.mpc_set_plant("aba", a.substeps)
bo.mpc_set_contact(bo.contact_defaults(kp=a.kp, kd=a.kd), bo.ground_under_feet(x0, 0.005))
vx = np.linspace(0.0, a.vx_max, B)
kf = BatchedOCP.keyframe
bo.mpc_set_timeline([[kf(0, "stand", 0.5),
                      kf(K_TROT, "trot", 0.8, ramp=True),
                      kf(K_FULL, "trot", 0.8, [v, 0, 0, 0, 0, 0]),
                      kf(K_WALK, "walk", 0.8, [0.5 * v, 0, 0, 0, 0, 0])] for v in vx])
bo.mpc_log_start(capacity=STEPS, dz_tol=0.10, cz_min=0.5)
bo.mpc_run(0, STEPS)
m = bo.mpc_metrics()
log = bo.mpc_log_read()
st = bo.mpc_timeline_state()
bo.close()
vbase = log["x_state"][:, :, R.nq]   # the base's forward velocity (base frame) after each step
rows = []
print("  vx_des finite  max_dz  min_cz not_solved first_out | vx after stand, ramp, trot, walk")
for b in range(B):
    ends = [float(vbase[k - 1, b]) for k in (K_TROT, K_FULL, K_WALK, STEPS)]
    rows.append({"vx_des": float(vx[b]), "finite": bool(m["first_nonfinite"][b] < 0), "max_dz": float(m["max_dz"][b]),
                 "min_cz": float(m["min_cz"][b]), "n_not_solved": int(m["n_not_solved"][b]),
                 "first_out": int(m["first_out"][b]), "vx_at_phase_end": ends, "last_segment": int(st["seg"][b])})
    r = rows[-1]
    print(f"  {r['vx_des']:6.3f} {str(r['finite']):>6} {r['max_dz']:7.4f} {r['min_cz']:7.4f} {r['n_not_solved']:10d} "
          f"{r['first_out']:9d} | " + ", ".join(f"{e:6.3f}" for e in ends), flush=True)
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps({"setup": vars(a), "problems": rows}, indent=1) + "\n")
