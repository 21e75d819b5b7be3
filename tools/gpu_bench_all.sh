#!/bin/bash
# Every bench line on one GPU: config 2 (with replay at 10k / 100k nodes, cycle and CPU baselines), 4, 5, 6.
#   bash tools/gpu_bench_all.sh <tag>      (from the repository root; results in $KG_OUT, default bench_out/)
set -o pipefail
TAG=${1:-b}
OUT=${KG_OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 500 python bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err" || exit 2
timeout -k 10 300 python bench.py --full --config 4 --no-cpu-baseline > "$OUT/bench4_$TAG.json" 2> "$OUT/bench4_$TAG.err" || exit 3
timeout -k 10 300 python bench.py --full --config 5 --steps 10 --warmup 2 > "$OUT/bench5_$TAG.json" 2> "$OUT/bench5_$TAG.err" || exit 4
timeout -k 10 300 python bench.py --full --config 6 --no-cpu-baseline > "$OUT/bench6_$TAG.json" 2> "$OUT/bench6_$TAG.err" || exit 5
for f in bench bench4 bench5 bench6; do python -c "
import json;d=json.loads(open('$OUT/${f}_$TAG.json').read().strip().splitlines()[-1])
print('$f', round(d['ms_per_step'],4), '%.4g'%d['value'], d['roofline'].get('kernel_avg_ms'), (d.get('cycle') or {}).get('ms_per_cycle'),
      (d.get('replay') or {}).get('pods_placed_per_s'), (d.get('replay_100k') or {}).get('pods_placed_per_s'), (d.get('cpu_baseline') or {}).get('value'))"; done
