#!/bin/bash
# usage: tools/ab_env.sh VAR v1 v2 ...   - alternate runs of the training bench under VAR=v (twice each), print ms per epoch and the per-kernel split
var=$1; shift
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for r in 1 2; do for v in "$@"; do echo "$var=$v"; env $var=$v python bench.py --full --steps 100 --warmup 5 --no-cpu-baseline --no-eval --no-secondary --no-quality --full-out "$OUT/ab_env_full.json" > /dev/null 2>&1; OUT=$OUT python -c "
import os,json
j=json.load(open(os.environ['OUT'] + '/ab_env_full.json')); k=j.get('kernels',{})
print(round(j['value']), round(j['ms_per_step'],3), {n:round(v['ms_per_step'],3) for n,v in k.items() if isinstance(v,dict) and 'ms_per_step' in v})"; done; done
