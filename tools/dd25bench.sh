#!/bin/bash
# Short timing of the 1520-bin configuration on the GPU box (through gpurun): sequences/s, ms per epoch, per-kernel ms.
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 250 python bench.py --full --dd 25 --ud-km 38 --steps 20 --no-cpu-baseline --no-secondary --no-quality --full-out "$OUT/dd25_full.json" > "$OUT/dd25.json" 2> "$OUT/dd25.err"; OUT=$OUT python -c "
import json, os; d=json.load(open(os.environ['OUT'] + '/dd25_full.json')); print(d['value'], d['ms_per_step']); k=d['kernels']
print({n: round(v['ms_per_step'],3) for n,v in k.items() if isinstance(v,dict) and 'ms_per_step' in v})"
