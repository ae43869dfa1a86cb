#!/usr/bin/env python
"""Filtered recommendation (models.compute_sub_topk_filtered, poi_score_topk_filtered) at the Gowalla shape (N = 100 k POIs, dim 128):
the top-20 among the POIs that pass a predicate, for pass fractions of 50 % / 10 % / 1 % / 0.1 %, calls of 1 / 64 / 4096 rows, the plain
score (BPR tables) and the spatial score (bins on the fly), one predicate shared by all rows against 64 distinct ones (row r uses
predicate r % 64: no two rows of a 32-row tile agree), without and with a 5 km radius.  The walk and the gather path are timed
separately (a radius is the gather path's alone).  Beside them, on the shared predicate, three things that exist without the feature:
  near     compute_sub_topk_near with the COMPLEMENT of the predicate as every row's exclusion list (and the same radius);
  topk     the plain compute_sub_topk(k = 20) over the same rows (no predicate: what a list costs at all);
  matrix   compute_sub_all_scores_device, the rows that fail masked to -inf, torch.topk (no radius) - and the share of rows on which
           its ids equal the fused call's.
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls -
as many as fill --window-ms - with ONE synchronisation at the end of the window, after a warm-up window; the path POI_FILTER_AUTO
takes with the predicate's pass count as the hint; and cost = (gather us / (rows * passing)) / (walk us / (ceil(rows / 32) * N)): what
one gathered candidate costs in walk cells IN THAT CELL - "filter_gather_cost" is this number where the two paths cross (DESIGN.md
section 27).  Also the time of poi_filter_build for 8 predicates over synthetic attributes.  Prints one JSON line.
    python tools/bench_filtered.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness
from poi_amd.models import PoiFilter

FRACTIONS = (0.5, 0.1, 0.01, 0.001)
N_DISTINCT = 64
RADIUS_KM = 5.0


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


def complement_lists(mask_row, n, device):
    """Every row's exclusion list = the POIs that FAIL the shared predicate: (off (n + 1), ids) int32 on the device."""
    gone = torch.nonzero(~mask_row).flatten().int()
    off = (torch.arange(n + 1, device=device, dtype=torch.int64) * gone.numel()).int()
    return off, gone.repeat(n).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 2 windows of 20 ms, rows 1 / 64")
    a = ap.parse_args()
    U, N, K, D = (4096, 10000, 20, 128) if a.quick else (50000, 100000, 20, 128)
    rows_of = (1, 64) if a.quick else (1, 64, 4096)
    if a.quick:
        a.repeats, a.window_ms = 2, 20.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, k=K, dim=D, radius_km=RADIUS_KM, distinct=N_DISTINCT), cells=[])
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
            m.set_coords(np.asarray(ds.coords, np.float64)[:N])
        score = "geo" if spatial else "plain"
        if not spatial:
            m.set_attributes(*pdata.synthetic_attributes(N, 200, seed=7), n_cat=200)
            preds = [dict(categories=[c]) for c in range(4)] + [dict(need=1), dict(any=6), dict(forbid=16), dict(categories=list(range(0, 200, 2)), need=2)]
            out["filter_build"] = dict(predicates=len(preds), counts=m.poi_filter(preds).counts.tolist(), **windows(lambda: m.poi_filter(preds), a.window_ms, a.repeats))
        gen = torch.Generator(device=m.device); gen.manual_seed(11)
        for frac in FRACTIONS:
            masks = torch.rand((N_DISTINCT, N), device=m.device, generator=gen) < frac
            shared, distinct = PoiFilter.from_masks(m, masks[:1]), PoiFilter.from_masks(m, masks)
            for n in rows_of:
                ids = rng.choice(U, n, replace=False).astype(np.int64)
                which = torch.arange(n, device=m.device, dtype=torch.int32) % N_DISTINCT
                t_topk = windows(lambda: m.compute_sub_topk(ids, K), a.window_ms, a.repeats)
                ex = complement_lists(masks[0], n, m.device)
                for preds_kind, filt, wh in (("shared", shared, None), ("distinct", distinct, which)):
                    passing = int(filt.counts.max())
                    for r_km in (None, RADIUS_KM):
                        call = lambda path: m.compute_sub_topk_filtered(ids, K, filt, which=wh, within_km=r_km, path=path, sync=False)
                        cell = dict(score=score, rows=n, frac=frac, preds=preds_kind, radius_km=r_km, passing=passing, topk=t_topk)
                        cell["gather"] = windows(lambda: call("gather"), a.window_ms, a.repeats)
                        gplan = m.ctx.last_plan("filter_splits")
                        if r_km is None:
                            cell["walk"] = windows(lambda: call("walk"), a.window_ms, a.repeats)
                            cell["splits"] = dict(walk=m.ctx.last_plan("filter_splits"), gather=gplan)
                            cell["cost"] = round((cell["gather"]["us"] / (n * max(passing, 1))) / (cell["walk"]["us"] / (((n + 31) // 32) * N)), 2)
                            assert torch.equal(call("walk"), call("gather"))
                        call("auto")
                        cell["auto_path"] = m.ctx.last_plan("filter_path")
                        if preds_kind == "shared":
                            cell["near"] = windows(lambda: m.compute_sub_topk_near(ids, K, within_km=r_km, exclude=ex, sync=False), a.window_ms, a.repeats)
                            if r_km is None:
                                keep = masks[0][None, :]

                                def matrix():
                                    return torch.topk(m.compute_sub_all_scores_device(ids).masked_fill(~keep, float("-inf")), K, dim=1).indices
                                cell["matrix"] = windows(matrix, a.window_ms, a.repeats)
                                cell["same_ids"] = round(float((call("auto") == matrix().int()).all(dim=1).float().mean()), 4)
                        best = min(cell[k]["us"] for k in ("walk", "gather") if k in cell)
                        print("[bench_filtered] %s rows %d frac %g %s radius %s: walk %s gather %.1f near %s matrix %s us" % (
                            score, n, frac, preds_kind, r_km, cell.get("walk", {}).get("us"), cell["gather"]["us"], cell.get("near", {}).get("us"),
                            cell.get("matrix", {}).get("us")), file=sys.stderr, flush=True)
                        cell["best_over_topk"] = round(best / t_topk["us"], 3)
                        out["cells"].append(cell)
                del ex
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
