#!/bin/bash
# One GPU-box visit: parity tests, smoke, bench (2a + 2b, --full), rocprofv3 kernel trace.  Logs -> the directory given.
set -u
OUT=${1:?usage: scripts/gpu_round.sh LOG_DIR}
mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== pytest -m gpu" ; timeout 900 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1; echo "pytest rc=$?"; tail -5 "$OUT/pytest_gpu.log"
echo "== smoke"; timeout 300 python __graft_entry__.py smoke > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?"; tail -2 "$OUT/smoke.log"
echo "== bench 2a"; timeout 600 python bench.py --full --steps 2000 --warmup 200 --fused > "$OUT/bench_2a.json" 2> "$OUT/bench_2a.err"; echo "rc=$?"; cat "$OUT/bench_2a.json"; tail -3 "$OUT/bench_2a.err"
echo "== bench 2b"; timeout 600 python bench.py --full --steps 2000 --warmup 200 --tasks 1024 --fused --no-cpu-baseline > "$OUT/bench_2b.json" 2> "$OUT/bench_2b.err"; echo "rc=$?"; cat "$OUT/bench_2b.json"; tail -3 "$OUT/bench_2b.err"
echo "== rocprofv3 kernel trace"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_r01" -o r01 -- python3 bench.py --steps 500 --warmup 50 --no-cpu-baseline > "$OUT/prof_bench.json" 2> "$OUT/prof.err"; echo "rc=$?"; cat "$OUT/prof_bench.json"
find "$OUT/prof_r01" -name "*stats*" | head; for f in $(find "$OUT/prof_r01" -name "*kernel_stats.csv"); do head -12 $f; done
