#!/bin/bash
# Validation pass on a GPU machine (OUT = the directory for the results): GM_TILE bitwise check + timing (tools/tile_bench), the -m gpu suite, the full bench line
cd "$(dirname "$0")/.."; OUT=${OUT:?set OUT to the directory for the results}; mkdir -p "$OUT"
export APRIL_LOG_LEVEL=${APRIL_LOG_LEVEL:-WARNING}
t0=$(date +%s)
timeout 300 tools/tile_bench 200 > $OUT/validate_tile_bench.txt 2>&1; echo "tile_bench rc=$?"; grep -E "^[a-z]|planner" $OUT/validate_tile_bench.txt
timeout 900 python -m pytest tests -m gpu -q -x --timeout 400 -p no:cacheprovider > $OUT/validate_pytest.log 2>&1
echo "pytest rc=$?  ($(( $(date +%s) - t0 )) s)"; tail -3 $OUT/validate_pytest.log
timeout 600 python bench.py --full > $OUT/validate_bench.json 2> $OUT/validate_bench.err; echo "bench rc=$?"
OUT=$OUT python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ['OUT'], 'validate_bench.json')))
for k in ('ms_per_step', 'steady', 'rtf_by_sessions_per_gpu', 'max_sessions_per_gpu_rtf_le_0.1_tested', 'replay_mismatch'):
    print(k, d.get(k))
c = d['config5_f16']; print('config5', c['f16']['ms_per_step'], c['f32']['ms_per_step'], c['f16_speedup_vs_f32'])
print(d['roofline']['avg_launch_us'], d['roofline']['frac'], d['roofline']['class_ms'])
PY
echo "total $(( $(date +%s) - t0 )) s"
