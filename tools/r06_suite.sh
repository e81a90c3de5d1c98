# the whole -m gpu suite as the driver runs it (+ durations), then the default bench line:  bash tools/r06_suite.sh <tag> <output dir> [nobench]
cd "$(dirname "$0")/.."
T=${1:-a}
O=${2:?usage: bash tools/r06_suite.sh <tag> <output dir> [nobench]}
timeout -k 10 1000 python -m pytest tests/ -x -q -m gpu --durations=15 > "$O/r06_suite_$T.log" 2>&1; rc=$?
echo "suite rc=$rc"; tail -4 "$O/r06_suite_$T.log"
if [ $rc -eq 0 ] && [ "$3" != "nobench" ]; then
  timeout -k 10 600 python bench.py --full > "$O/r06_bench_$T.log" 2> "$O/r06_bench_$T.err"; echo "bench rc=$?"
  cp "$(python -c 'import json, sys; print(json.loads(open(sys.argv[1]).read().splitlines()[-1])["detail"])' "$O/r06_bench_$T.log")" "$O/r06_bench_${T}_detail.json"
  tail -c 4200 "$O/r06_bench_$T.log"
fi
