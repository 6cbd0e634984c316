#!/bin/bash
# The full benchmark (bench.py --full: headline, config 5, secondary rows, accumulate, mc_step); line and detail land in ${OUT:-bench_out}/
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
( time timeout 1200 python bench.py --full > "$OUT/full_bench_line.json" 2> "$OUT/full_bench.err" ) 2>&1 | grep real
cp bench_detail.json "$OUT/full_bench_detail.json"
python - <<PY
import json
d=json.load(open("$OUT/full_bench_line.json"))
print(d["config"].get("device"), d["roofline"]["frac"], d["roofline"]["frac_hbm_min_over_steps"], d["roofline"]["placement"])
for r in d["secondary"]: print(r)
print(d["config5"]); print(d["accumulate"]); print(d.get("mc_step"))
PY
wc -c "$OUT/full_bench_line.json"
