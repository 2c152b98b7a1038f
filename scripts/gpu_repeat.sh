# Run-to-run spread of the default (config 3) bench line (--full: with its
# kernel clock and roofline) on one box.  Outputs under $OUT (default
# bench_out/ in the repository).
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
T=${TAG:-repeat}
: > "$OUT/${T}.jsonl"
for i in 1 2 3 4 5; do
  echo "== run $i"
  timeout -k 10 120 python bench.py --full --no-cpu-baseline > "$OUT/${T}_$i.json" 2> "$OUT/${T}_$i.err" || exit $?
  python -c "import json,sys; d=json.load(open(sys.argv[1])); print(json.dumps({'run': int(sys.argv[2]), 'value': d['value'], 'kernel_ms': d['config']['kernel_ms'], 'ms_per_step': d['ms_per_step'], 'frac': d['roofline']['frac']}))" "$OUT/${T}_$i.json" $i | tee -a "$OUT/${T}.jsonl"
done
