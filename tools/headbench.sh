#!/bin/bash
# Short timing of the training launch on the GPU box (through gpurun): throughput, epoch time and the per-kernel regions.
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 300 python bench.py --full --steps 100 --no-cpu-baseline --no-secondary --no-quality --eval-steps 1 --full-out "$OUT/bench_a_full.json" > "$OUT/bench_a.json" 2> "$OUT/bench_a.err"; OUT=$OUT python -c "
import json, os; d=json.load(open(os.environ['OUT'] + '/bench_a_full.json')); print(d['value'], d['ms_per_step']);
for k,v in d['kernels'].items(): print(k, round(v['ms_per_step'],3), round(1e3*v['avg_ms'],1), v.get('frac'))"
