# Full GPU parity suite, smoke, bench (--full) + rocprofv3 kernel stats.  Logs go to $OUT_DIR.
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
rc=$?; echo "pytest exit $rc" >> "$O/pytest_gpu.log"
case "$rc" in 0|1) ;; *) exit 1;; esac
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > "$O/bench.log" 2>&1 || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$O/prof" -o run -- python3 bench.py > "$O/prof.log" 2>&1 || exit 1
echo done
