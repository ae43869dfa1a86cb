#!/bin/bash
# usage: tools/ab_eval.sh <POI_SCORE_DBG values...>   - one bench run per value, prints the evaluation timings
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for d in "$@"; do
  POI_SCORE_DBG=$d python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --full-out "$OUT/ab_eval_full.json" > /dev/null 2>&1; D=$d OUT=$OUT python -c "
import sys,json,os
j=json.load(open(os.environ['OUT'] + '/ab_eval_full.json')); e=j['eval']
print('dbg', os.environ['D'], 'eval ms', round(e['ms_per_eval'],2), 'score', round(e['ms_score_topk_per_eval'],2), 'predict', round(e['ms_predict_per_eval'],2), 'frac', round(e['score_topk_frac_of_f32_mfma_peak'],3))"
done
