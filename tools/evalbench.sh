#!/bin/bash
# Short timing of the evaluation pass on the GPU box (through gpurun): users/s, ms per evaluation, scoring kernel share.
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 400 python bench.py --full --steps 20 --eval-steps 5 --no-cpu-baseline --no-secondary --no-quality --full-out "$OUT/bench_e_full.json" > "$OUT/bench_e.json" 2> "$OUT/bench_e.err"; OUT=$OUT python -c "
import json, os; d=json.load(open(os.environ['OUT'] + '/bench_e_full.json')); e=d['eval']; print(d['eval_users_per_s'], e['ms_per_eval'], e['ms_score_topk_per_eval'], e['score_topk_equivalent_frac_of_f32_mfma_peak'], e['ms_per_eval_unseeded'], e['recall_at_20_after_timed_training'])"
