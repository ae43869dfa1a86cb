#!/usr/bin/env python
"""Candidate generation (models.compute_sub_candidates, poi_score_candidates) at the Gowalla shape (N = 100 k POIs, dim 128, 50 k users):
the exact top-k for k = 100 / 1000 / 4096 over calls of 1 / 64 / 4096 rows, the plain score (BPR tables) and the spatial score (bins on
the fly).  Beside it, in the same process:
  torch    the yardstick: compute_sub_all_scores_device + torch.topk(k) over the same rows (rows within 2 GiB of scores at a time),
           which must pick the same ids on rows without exact ties;
  topk     compute_sub_topk(k = 20) over the same rows: what a long list costs over a short one;
  stages   from the library's event timing over the fused calls: "score_rows", each digit pass ("select_pass0" / 1 / 2),
           "select_collect" and "select_sort", milliseconds per call.
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls -
as many as fill --window-ms - with ONE synchronisation at the end of the window, after a warm-up window; the ratio fused / torch of the
medians; the plan taken; the share of rows on which torch.topk picks the same ids.  Prints one JSON line.
    python tools/bench_candidates.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness

STAGES = ("score_rows", "select_pass0", "select_pass1", "select_pass2", "select_collect", "select_sort")


def windows(fn, window_ms, repeats):
    """A window is a FIXED number of chained calls and one synchronisation: the number that fills window_ms at the duration of one
    synchronised call."""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    calls = max(1, min(10000, int(window_ms / max((time.perf_counter() - t0) * 1e3, 1e-3))))

    def one():
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2), calls=calls)


def torch_route(m, ids, k):
    step = max(1, (1 << 29) // m.n_item)
    return torch.cat([torch.topk(m.compute_sub_all_scores_device(ids[o:o + step]), k, dim=1)[1] for o in range(0, len(ids), step)]).int()


def stage_times(m, fn, calls=5):
    """Milliseconds per call of every stage, from HIP events around the kernels of `calls` calls."""
    m.ctx.timing(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {s: round(m.ctx.timing_get(s)[0] / calls, 4) for s in STAGES}
    m.ctx.timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, dim=D), cells=[])
    rng = np.random.default_rng(3)
    for spatial in (False, True):
        p = harness.default_params()
        p.update(latent_size=D, gru=2 if spatial else 0)
        m = harness.build_model(ds, p, seed=5)
        m.update_trained_items()
        if spatial:
            m.update_trained_dists()
            m.update_trained_users(torch.rand((U, D), device=m.device) - 0.5)
            m.update_trained_sus(torch.rand((U, m.n_dist + 1), device=m.device))
        else:
            m.update_trained_users()
        score = "geo" if spatial else "plain"
        for n in (1, 64, 4096):
            ids = rng.choice(U, n, replace=False).astype(np.int64)
            t_topk = windows(lambda: m.compute_sub_topk(ids, 20), a.window_ms, a.repeats)
            for k in (100, 1000, 4096):
                run = lambda: m.compute_sub_candidates(ids, k, sync=False)
                fused = windows(run, a.window_ms, a.repeats)
                plan = {key: m.ctx.last_plan(key) for key in ("select_path", "select_splits", "select_chunks", "select_rows_per_chunk")}
                ref = windows(lambda: torch_route(m, ids, k), a.window_ms, a.repeats)
                agree = float((m.compute_sub_candidates(ids, k) == torch_route(m, ids, k)).all(dim=1).float().mean())
                print("[bench_candidates] %s rows %d k %d: fused %.1f us, torch.topk %.1f us, same ids %.4f" % (score, n, k, fused["us"], ref["us"], agree),
                      file=sys.stderr, flush=True)
                out["cells"].append(dict(score=score, rows=n, k=k, fused=fused, torch=ref, topk20=t_topk, plan=plan, stages_ms=stage_times(m, run),
                                         ratio=round(fused["us"] / ref["us"], 3), same_ids=round(agree, 4)))
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
