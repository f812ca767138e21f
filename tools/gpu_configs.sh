#!/bin/bash
# One bench line (--full: CPU baseline, host_io, roofline at every batch) per BASELINE config
#  and the interior-point line at the headline config; JSON lines
# into $OUT_DIR/configs.jsonl.
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
: > "$O/configs.jsonl"
run() {
  timeout -k 10 400 python bench.py --full "$@" > "$O/cfg.log" 2>&1 || { tail -20 "$O/cfg.log"; exit 1; }
  tail -1 "$O/cfg.log" >> "$O/configs.jsonl"
}
run --robot go2 --dynamics centroidal_vel --nodes 20 --batch 1024 --steps 40 --warmup 2          # config 1
run --robot go2 --dynamics whole_body_rnea --nodes 20 --batch 1 --steps 40 --warmup 2            # config 2 (one problem)
run --robot b2 --dynamics whole_body_aba --nodes 40 --batch 256 --steps 40 --warmup 2            # config 3
run --robot b2g --dynamics whole_body_acc --nodes 50 --batch 1024 --steps 40 --warmup 2          # config 4
run --solver fatrop --steps 10 --warmup 1 --host-io-steps 0                                     # headline, Fatrop branch (ip_stats: the 11th MPC step)
cut -c1-200 "$O/configs.jsonl"
