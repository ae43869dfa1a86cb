#!/usr/bin/env python
"""Label recommendation (models.recommend_labels, poi_score_topk_labels) at the Gowalla shape (N = 100 k POIs, dim 128, 200 bins): the
top-10 labels by softmax mass for calls of 1 / 64 / 4096 rows, the plain score (BPR tables) and the spatial score (bins on the fly),
under three labellings:
  zipf    37 categories of very unequal size (accumulators in LDS at the default "labels_lds_kb");
  grid    the 1 km cells of data.grid_labels over the POI coordinates (thousands of labels: the global accumulator);
  five    5 labels (LDS; 32 lanes of a row meet on 5 addresses).
Beside every cell, on the same rows, three routes that exist without the feature:
  matrix    compute_sub_all_scores_device, a float64 logsumexp per row, exp(s - lse) scatter-added by label (index_add), top-10 - the
            (n, n_item) matrix the feature avoids; `same`: the share of the rows with clear gaps (adjacent log-masses of the matrix
            route's top 11 at least 1e-5 max(1, max |score|) apart) on which both routes list the same labels in the same order;
  capped    compute_sub_topk_capped(per = 1) at k = 10: the label-level answer that existed, by the single best POI;
  topk      the plain compute_sub_topk at k = 20: what a POI list costs.
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls
with ONE synchronisation at the end of the window, after a warm-up window; and, from the context's event timing over separate calls,
the max pass, the accumulating walk and the finish kernel on their own ("max_us" / "walk_us" / "finish_us").  --home both times the
LDS labellings with the accumulators forced into global memory too ("global").  Prints one JSON line.
    python tools/bench_labels.py [--repeats N] [--window-ms T] [--quick] [--home both]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness

K = 10


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


def matrix_route(m, ids, lab, n_label, k):
    """(labels (n, k), clear (n) bool) from the score matrix: float64 logsumexp, index_add by label, top-k."""
    full = m.compute_sub_all_scores_device(ids).double()
    p = torch.exp(full - torch.logsumexp(full, dim=1, keepdim=True))
    mass = torch.zeros((full.shape[0], n_label + 1), dtype=torch.float64, device=full.device)
    mass.index_add_(1, torch.where(lab >= 0, lab, torch.full_like(lab, n_label)).long(), p)
    kk = min(k + 1, n_label)
    v, order = torch.topk(mass[:, :n_label], kk, dim=1)
    lv = torch.log(v)
    tol = 1e-5 * max(1.0, float(full.abs().max()))
    clear = ((lv[:, :-1] - lv[:, 1:]) >= tol).all(dim=1) if kk > 1 else torch.ones(full.shape[0], dtype=torch.bool, device=full.device)
    return order[:, :k].int(), clear


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 2 windows of 10 ms, rows 1 / 64")
    ap.add_argument("--home", choices=("auto", "both"), default="auto")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    rows_of = (1, 64) if a.quick else (1, 64, 4096)
    if a.quick:
        a.repeats, a.window_ms = 2, 10.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    coords = np.asarray(ds.coords, np.float64)[:N]
    cells_lab, n_cells, _ = pdata.grid_labels(coords, 1.0)
    labelings = dict(zipf=pdata.synthetic_attributes(N, 37, seed=7)[0], grid=cells_lab, five=(np.arange(N) * 7919 % 5).astype(np.int32))
    out = dict(shape=dict(users=U, pois=N, k=K, dim=D, grid_labels=n_cells), cells=[])
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
            m.set_coords(coords)
        score = "geo" if spatial else "plain"
        for name, lab in labelings.items():
            labels = m.poi_labels(lab)
            for n in rows_of:
                ids = rng.choice(U, n, replace=False).astype(np.int64)
                call = lambda: m.recommend_labels(ids, min(K, labels.n_label), labels, sync=False)
                cell = dict(score=score, rows=n, labels=name, n_label=labels.n_label)
                for home in (("auto", "global") if a.home == "both" and name != "grid" else ("auto",)):
                    m.ctx.set_option("labels_lds_kb", 40 if home == "auto" else 0)
                    r = dict(windows(call, a.window_ms, a.repeats))
                    r["home"], r["splits"] = m.ctx.last_plan("labels_home"), m.ctx.last_plan("labels_splits")
                    m.ctx.timing(True)
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    for key in ("labels_max", "labels_walk", "labels_finish"):
                        ms, cnt = m.ctx.timing_get(key)
                        r[key.replace("labels_", "") + "_us"] = round(1e3 * ms / cnt, 2) if cnt else None
                    m.ctx.timing(False)
                    cell["fused" if home == "auto" else "global"] = r
                m.ctx.set_option("labels_lds_kb", 40)
                fused = call()[0]
                cell["capped"] = windows(lambda: m.compute_sub_topk_capped(ids, min(K, labels.n_label), labels, per=1, sync=False), a.window_ms, a.repeats)
                cell["topk"] = windows(lambda: m.compute_sub_topk(ids, 20), a.window_ms, a.repeats)
                if n <= 64 or name == "zipf":                                        # (thousands of rows: 3.2 GB of float64 per call - one labelling)
                    cell["matrix"] = windows(lambda: matrix_route(m, ids, labels.labels, labels.n_label, min(K, labels.n_label)), a.window_ms, a.repeats)
                    ref, clear = matrix_route(m, ids, labels.labels, labels.n_label, min(K, labels.n_label))
                    cell["clear"] = round(float(clear.float().mean()), 4)
                    cell["same"] = round(float((ref[clear] == fused[clear]).all(dim=1).float().mean()), 4) if bool(clear.any()) else None
                g = cell["fused"]
                print("[bench_labels] %s rows %d %s (%d labels, home %d, splits %d): labels %.1f (max %s walk %s finish %s) | matrix %s (clear %s same %s) capped %.1f topk %.1f us"
                      % (score, n, name, labels.n_label, g["home"], g["splits"], g["us"], g["max_us"], g["walk_us"], g["finish_us"],
                         cell.get("matrix", {}).get("us"), cell.get("clear"), cell.get("same"), cell["capped"]["us"], cell["topk"]["us"]), file=sys.stderr, flush=True)
                out["cells"].append(cell)
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
