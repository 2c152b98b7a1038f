# Quick GPU check: pytest -m gpu, then the three bench lines (--full) without
# the CPU baseline.  Run from anywhere; TAG names the outputs under $OUT
# (default bench_out/ in the repository).
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
T=${TAG:-quick}
echo "== pytest gpu"; timeout -k 10 600 python -u -m pytest tests -m gpu -x -v -s --timeout 120 --timeout-method thread > "$OUT/${T}_pytest_gpu.log" 2>&1; rc=$?; tail -3 "$OUT/${T}_pytest_gpu.log"; [ $rc -eq 0 ] || { grep -E "FAILED|Error|assert" "$OUT/${T}_pytest_gpu.log" | head -20; exit $rc; }
for w in shadow path flat; do
echo "== bench $w"; timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline > "$OUT/${T}_bench_$w.json" 2> "$OUT/${T}_bench_$w.err"; rc=$?; python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(d['value'],d['ms_per_step'],d['config']['kernel_ms'],d['roofline']['counts'])" "$OUT/${T}_bench_$w.json"; [ $rc -eq 0 ] || exit $rc
done
