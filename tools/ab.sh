#!/bin/bash
# usage: tools/ab.sh <filter> <dbg values...>   - bench one train step per POI_TE_DBG value, print matching kernels
flt=$1; shift
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for d in "$@"; do
  POI_TE_DBG=$d python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-eval --full-out "$OUT/ab_full.json" > /dev/null 2>&1; D=$d F=$flt OUT=$OUT python -c "
import sys,json,os
j=json.load(open(os.environ['OUT'] + '/ab_full.json')); k=j.get('kernels',{})
print('dbg', os.environ['D'], round(j['ms_per_step'],3), {n:round(v['ms_per_step'],3) for n,v in k.items() if os.environ['F'] in n})"
done
