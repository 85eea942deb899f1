#!/bin/bash
# selected GPU tests, bench, kernel-trace stats + per-update tail breakdown
#   tools/gpu/tests_bench_trace.sh TAG [pytest -k expression]
set -o pipefail
cd "$(dirname "$0")/../.."
export OUT=${OUT:-bench_out}   # where the logs and results go
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-r03}
SEL=${2:-}
if [ -n "$SEL" ]; then
  timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 900 --timeout-method thread -k "$SEL" > $OUT/pytest_${TAG}.log 2>&1 || { echo "pytest failed"; tail -40 $OUT/pytest_${TAG}.log; exit 1; }
  tail -3 $OUT/pytest_${TAG}.log
fi
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu > $OUT/bench_${TAG}.log 2>&1 || { echo "bench failed"; tail -20 $OUT/bench_${TAG}.log; exit 1; }
tail -1 $OUT/bench_${TAG}.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); c=d["config"]; r=d["roofline"]; print("value %.4g ms/step %.3f c0 %.3f never %.1f over %.1f spills %.1f" % (d["value"], d["ms_per_step"], r["kernel_ms"], c["births_never_placed_per_update"], c["births_overwritten_per_update"], c["spills_per_update"]))'
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt_${TAG} -o run -- python bench.py --steps 40 --warmup 2 --no-cpu --long-updates 0 > $OUT/kt_${TAG}.log 2>&1 || { echo "kernel trace failed"; tail -20 $OUT/kt_${TAG}.log; exit 1; }
python tools/tail_summary.py $(ls $OUT/kt_${TAG}/*/*kernel_trace.csv $OUT/kt_${TAG}/*kernel_trace.csv 2>/dev/null | head -1) > $OUT/${TAG}_tail_per_update.txt
cat $OUT/${TAG}_tail_per_update.txt
cp $(ls $OUT/kt_${TAG}/*/*kernel_stats.csv $OUT/kt_${TAG}/*kernel_stats.csv 2>/dev/null | head -1) $OUT/${TAG}_kernel_stats_bench.csv || true
