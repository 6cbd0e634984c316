cd "$(dirname "$0")/.." || exit 1; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for t in f g h; do
  timeout 900 python bench.py --full > $OUT/r06_${t}_bench_line.json 2> /dev/null
  python - <<PY
import json
l=json.loads(open('$OUT/r06_${t}_bench_line.json').read()); r=l['roofline']
print('${t}', l['value'], r['frac'], r.get('frac_from_ms_per_step'), r.get('frac_hbm_min_over_steps'), l['config']['device'], l['config5']['value'], l['accumulate']['frac_hbm'])
PY
done
