#!/bin/bash
# GPU round check: parity tests, smoke, bench line (--full), rocprofv3 kernel stats and the
# two PMC passes (FETCH_SIZE / WRITE_SIZE, separate runs) for k_admm traffic.
# Usage (from the repository root): [OUT_DIR=dir] bash tools/gpu_round.sh [tag]
set -o pipefail
R=$(pwd)
TAG=${1:-run}
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
  rc=$?
  echo "pytest exit $rc" >> "$O/pytest_gpu.log"
  case "$rc" in 0|1) ;; *) echo "stopping after pytest rc=$rc"; exit 1;; esac
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || exit 1
  timeout -k 10 300 python tools/parity_report.py > "$O/parity_report.log" 2>&1 || exit 1
fi
timeout -k 10 600 python bench.py --full > "$O/bench.log" 2>&1 || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$O/prof" -o run -- python3 bench.py > "$O/prof.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex 'k_admm<' --output-format csv -d "$R/$O/pmc_fetch" -o run -- python3 bench.py --steps 2 --warmup 0 > "$O/pmc_fetch.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex 'k_admm<' --output-format csv -d "$R/$O/pmc_write" -o run -- python3 bench.py --steps 2 --warmup 0 > "$O/pmc_write.log" 2>&1 || exit 1
python tools/pmc_traffic.py "$O/pmc_fetch" "$O/pmc_write" "$O/pmc_fetch.log" "$O/admm_traffic.json"
