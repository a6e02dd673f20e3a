# quick headline check: parity b32, no sides / oracle / cpu baseline
OUT=$(mktemp)
python bench.py --full --steps 20 --warmup 5 --no-side --no-parity --no-parity-at-batch --no-cpu-baseline 2>/dev/null | tail -1 > "$OUT"
python - "$OUT" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(d['value'], d['ms_per_step'])
for k in d['roofline'].get('kernels', []): print(f"{k['name']:36s} {k['ms_per_step']:.3f} {k.get('executed_tflops')}")
PY
