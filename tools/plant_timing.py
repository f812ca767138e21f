"""Kernel time of the MPC loop's plant (k_plant, k_plant.hip) beside k_mpc_finish at the headline shape.

Two halves, because a kernel's own time comes from the profiler's kernel trace, in a run of its own:

  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \
      python tools/plant_timing.py run --mode aba --substeps 4 [--contact] [robot dynamics N B]
      an MPC loop (3 warm-up steps + 10) with the plant as given; eager launches (no_mpc_graph), so
      every launch is one dispatch of the trace.  The plant runs on the solved iterate of each step.
      --contact adds the ground contact and joint PD of mpc_set_contact (k_plant's contact
      instantiation; profiles/plant/plant_contact_timing.json).  --log switches the rollout log on
      (mpc_log_start, one slot per step), so that every step also dispatches k_mpc_record
      (profiles/plant/record_timing.json).  --timeline sets a three-keyframe timeline per problem
      (mpc_set_timeline: trot with a velocity ramp, then walk), so that k_mpc_prepare evaluates it at
      every step (profiles/plant/timeline_timing.json, parsed with @k_mpc_prepare).
  python tools/plant_timing.py parse LABEL[@KERNEL]=DIR [LABEL[@KERNEL]=DIR ...] [--out FILE]
      per label the median / min / max duration of the last 10 k_plant or k_mpc_finish dispatches
      of DIR's *kernel_trace.csv, as one JSON; @KERNEL picks the dispatches whose name contains
      KERNEL instead ("k_mpc_record(" and k_mpc_finish of one --log run; the bracket keeps
      k_mpc_record_start, the one launch of mpc_log_start, out).

The PINOLOCO_LIB environment variable selects another build of the library (e.g. one built with
PL_HIPCC_DEFS=-DPL_PLANT_LANES=64) for a same-box comparison of the mapping.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "pino-locoman_amd"))
WARM, STEPS = 3, 10


def run(args):
    from pinoloco import _lib, robots
    from pinoloco.ocp import BatchedOCP
    from pinoloco.synthetic import build_batch
    rob, dyn, N, B = args.shape[0], args.shape[1], int(args.shape[2]), int(args.shape[3])
    R = robots.ROBOTS[rob]()
    R.set_gait_sequence("trot", 0.8)
    lay, P, X, XS, T0 = build_batch(R, dyn, N, B, 0)
    bo = BatchedOCP(R, dyn, N, batch=B, device=0, debug_paths=("no_mpc_graph",))
    bo.set_params(P)
    bo.set_x(X)
    bo.init_solver()
    bo.mpc_setup(XS, T0)
    bo.mpc_set_plant(args.mode, args.substeps)
    if args.mode == "aba":  # a push on every problem: the wrench is read either way
        bo.mpc_set_disturbance(base_wrench=np.random.default_rng(5).normal(size=(B, 6)) * 10.0)
    if args.contact:
        # the ground under each problem's own feet.  The defaults of this tool are a soft, lightly
        # damped ground (5 cm, zeta 0.05) that stays inside the explicit damping limit at one
        # substep too, so that every timed run steps finite states; the kernel's work per substep
        # does not depend on the values.
        c = bo.contact_defaults(penetration=args.penetration, zeta=args.zeta, kp=40.0, kd=1.0)
        bo.mpc_set_contact(c, bo.ground_under_feet(XS, args.penetration))
    if args.log:
        bo.mpc_log_start(capacity=WARM + STEPS, dz_tol=0.1, cz_min=0.5)
    if args.timeline:
        vx = P[:, lay.poff["base_vel_des"][0]]
        kf = BatchedOCP.keyframe
        bo.mpc_set_timeline([[kf(0, "trot", 0.8, [0, 0, 0, 0, 0, 0], ramp=True), kf(8, "trot", 0.8, [v, 0, 0, 0, 0, 0]),
                              kf(11, "walk", 0.6, [0.5 * v, 0, 0, 0, 0, 0], t_shift=0.05)] for v in vx])
    for k in range(WARM + STEPS):
        bo.mpc_step(k)
    xs = bo.mpc_state()
    out = {"mode": args.mode, "substeps": args.substeps, "contact": bool(args.contact), "shape": args.shape,
           "lib": _lib.LIB_PATH, "lib_src_sha256": _lib.build_sha(), "finite": bool(np.all(np.isfinite(xs)))}
    if args.timeline:
        out["timeline_last_segment"] = sorted(set(bo.mpc_timeline_state()["seg"].tolist()))
    if args.log:
        sz = bo.mpc_log_sizes()
        out["log"] = {k: sz[k] for k in ("row", "recorded", "dropped")}
        out["log_last_state_is_state"] = bool(np.array_equal(bo.mpc_log_read(WARM + STEPS - 1, 1)["x_state"][0], xs,
                                                            equal_nan=True))
    if args.contact:
        out["feet_on_ground"] = float(bo.mpc_get_contact()["anchors"][:, :, 2].mean())
    print(json.dumps(out))
    bo.close()


def parse(args):
    out = {}
    for item in args.dirs:
        label, d = item.split("=", 1)
        label, _, pick = label.partition("@")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"{label}: expected one kernel trace under {d}, found {files}")
        ns, name = [], None
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                kn = row["Kernel_Name"]
                if (pick in kn) if pick else ("k_plant" in kn or "k_mpc_finish" in kn):
                    name = kn
                    ns.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                               int(row["Workgroup_Size_X"]), int(row["Grid_Size_X"]), int(row["Scratch_Size"])))
        if len(ns) != WARM + STEPS:
            raise SystemExit(f"{label}: {len(ns)} plant dispatches, expected {WARM + STEPS}")
        ns.sort()
        t = np.array([x[1] for x in ns[WARM:]]) / 1e3
        out[label] = {"kernel": name, "dispatches": len(t), "median_us": float(np.median(t)), "min_us": float(t.min()),
                      "max_us": float(t.max()), "workgroup": ns[0][2], "grid": ns[0][3], "scratch_bytes_per_lane": ns[0][4]}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
r = sub.add_parser("run")
r.add_argument("--mode", default="aba", choices=["aba", "nominal"])
r.add_argument("--substeps", type=int, default=1)
r.add_argument("--contact", action="store_true", help="ground contact and joint PD (mpc_set_contact), aba only")
r.add_argument("--log", action="store_true", help="the rollout log on: k_mpc_record after every step")
r.add_argument("--timeline", action="store_true", help="a gait and command timeline on: k_mpc_prepare evaluates it")
r.add_argument("--penetration", type=float, default=0.05)
r.add_argument("--zeta", type=float, default=0.05)
r.add_argument("shape", nargs="*", default=["b2g", "whole_body_rnea", "50", "1024"])
p = sub.add_parser("parse")
p.add_argument("dirs", nargs="+")
p.add_argument("--out", default=None)
a = ap.parse_args()
run(a) if a.cmd == "run" else parse(a)
