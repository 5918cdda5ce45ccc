#!/bin/bash
# A/B of branch-stream count and lanes on the f16 detect benches (bench.py --full: device and predict img/s).
# OUT: the directory the result lines go to (default bench_out/ab2)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out/ab2}
mkdir -p "$OUT"
for m in s n; do
  for cfg in "YM_BRANCHES=4 L=1" "YM_BRANCHES=3 L=1" "YM_BRANCHES=2 L=1" "YM_BRANCHES=4 L=2"; do
    br=$(echo $cfg | sed 's/YM_BRANCHES=\([0-9]\).*/\1/'); l=$(echo $cfg | sed 's/.*L=//')
    YM_BRANCHES=$br timeout -k 10 200 python bench.py --full --model $m --no-cpu --no-roofline --steps 200 --lanes $l > "$OUT/${m}_${br}_${l}.json" 2>/dev/null || exit 1
    python -c "import json; d=json.load(open('$OUT/${m}_${br}_${l}.json')); print('$m branches=$br lanes=$l', d['value'], d['device_images_per_s'])"
  done
done
