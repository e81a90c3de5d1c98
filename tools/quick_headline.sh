# quick check of the headline path: bit-identity / oracle tests of the render kernels, then the bench line (no extra legs)
#   bash tools/quick_headline.sh <output dir>
O=${1:?usage: bash tools/quick_headline.sh <output dir>}
mkdir -p "$O"
timeout -k 10 400 python -m pytest tests/test_density_sliced_gpu.py tests/test_render_static_gpu.py tests/test_occupancy_gpu.py tests/test_reference_fixtures_gpu.py -x -q -m gpu > "$O/t1.log" 2>&1
rc=$?
tail -3 "$O/t1.log"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --no-extra-legs --train-steps 0 --cpu-rays 0 > "$O/b1.log" 2>&1 || { tail -5 "$O/b1.log"; exit 1; }
python - "$O/b1.log" <<PY
import json, sys
l=[x for x in open(sys.argv[1]) if x.startswith("{")][-1]
d=json.loads(l)
print(d["value"], d["ms_per_step"], [(k[0], round(k[1],4)) for k in d["kernels"]])
PY
