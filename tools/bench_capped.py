#!/usr/bin/env python
"""Capped recommendation (models.compute_sub_topk_capped, poi_score_topk_capped) at the Gowalla shape (N = 100 k POIs, dim 128): the
top-20 with at most `per` POIs of one label, for calls of 1 / 64 / 4096 rows, the plain score (BPR tables) and the spatial score (bins
on the fly), per = 1 / 2 / 5, without and with a 10 % predicate, under four labelings:
  zipf    37 categories of very unequal size;
  grid    the 1 km cells of data.grid_labels over the POI coordinates (thousands of labels);
  five    5 labels - the lists cannot fill (5 * per < 20): the fill-gate case, run with the fill table AND without it ("nofill");
  by_id   8 labels equal to id * 8 // N - clustered by id, so that a wave's quarter of a slice holds one label: the per-wave slow path.
Beside every cell, on the same rows, three routes that exist without the feature:
  topk      compute_sub_topk_filtered with the same predicate (without one: the plain compute_sub_topk) at k = 20 - what a list costs
            without a cap;
  cand      compute_sub_candidates(k = 4096) plus the greedy pass in torch (a stable sort by label gives every candidate the number of
            same-label candidates in front of it), and `short`: the share of rows whose list differs from the fused one - 4096 was
            not deep enough (no predicate only: the candidate entry takes none);
  matrix    compute_sub_all_scores_device, the rows that fail masked to -inf, a full torch.sort and the same greedy pass (at 4096
            rows under the zipf labelling and per = 2 only: gigabytes of sort keys per call).
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls
with ONE synchronisation at the end of the window, after a warm-up window; and, from the context's event timing over separate calls,
the walk kernel and the slice merge on their own ("walk_us" / "merge_us"; no merge outside the split regime).  Also poi_labels_build
for the grid labelling.  Prints one JSON line.
    python tools/bench_capped.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness
from poi_amd.models import PoiFilter

PERS = (1, 2, 5)
DEPTH = 4096


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


def greedy(ids, lab, per, k):
    """ids (n, depth) ranked candidates (-1: none), lab (N) device labels -> the capped first k (n, k), -1 fill."""
    n, depth = ids.shape
    there = ids >= 0
    l = lab[ids.clamp(min=0).long()]
    key = torch.where(there & (l >= 0), l.long(), torch.full_like(l, -1).long())
    order = torch.sort(key, dim=1, stable=True).indices                       # same-label candidates side by side, in rank order
    ks = key.gather(1, order)
    pos = torch.arange(depth, device=ids.device).expand(n, depth)
    start = torch.where(torch.cat([torch.ones_like(ks[:, :1], dtype=torch.bool), ks[:, 1:] != ks[:, :-1]], 1), pos, torch.zeros_like(pos))
    before = torch.zeros_like(pos).scatter_(1, order, pos - torch.cummax(start, 1).values)
    keep = there & ((key < 0) | (before < per))
    rank = torch.cumsum(keep.long(), 1) - 1
    out = torch.full((n, k + 1), -1, dtype=ids.dtype, device=ids.device)
    out.scatter_(1, torch.where(keep & (rank < k), rank, torch.full_like(rank, k)), ids)
    return out[:, :k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 2 windows of 10 ms, rows 1 / 64")
    a = ap.parse_args()
    U, N, K, D = (4096, 10000, 20, 128) if a.quick else (50000, 100000, 20, 128)
    rows_of = (1, 64) if a.quick else (1, 64, 4096)
    if a.quick:
        a.repeats, a.window_ms = 2, 10.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    coords = np.asarray(ds.coords, np.float64)[:N]
    cells_lab, n_cells, _ = pdata.grid_labels(coords, 1.0)
    labelings = dict(zipf=pdata.synthetic_attributes(N, 37, seed=7)[0], grid=cells_lab, five=(np.arange(N) * 7919 % 5).astype(np.int32),
                     by_id=(np.arange(N, dtype=np.int64) * 8 // N).astype(np.int32))
    out = dict(shape=dict(users=U, pois=N, k=K, dim=D, depth=DEPTH, grid_labels=n_cells), cells=[])
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
        gen = torch.Generator(device=m.device); gen.manual_seed(11)
        mask = torch.rand((1, N), device=m.device, generator=gen) < 0.1
        filt = PoiFilter.from_masks(m, mask)
        if not spatial:
            out["labels_build"] = dict(labels=n_cells, **windows(lambda: m.poi_labels(cells_lab, n_cells), a.window_ms, a.repeats))
        for name, lab in labelings.items():
            built = {None: m.poi_labels(lab), filt: m.poi_labels(lab, filt=filt)}
            for n in rows_of:
                ids = rng.choice(U, n, replace=False).astype(np.int64)
                for f in (None, filt):
                    labels = built[f]
                    if f is None:
                        t_topk = windows(lambda: m.compute_sub_topk(ids, K), a.window_ms, a.repeats)
                        cand = lambda: m.compute_sub_candidates(ids, min(DEPTH, N), sync=False)
                        keep = None
                    else:
                        t_topk = windows(lambda: m.compute_sub_topk_filtered(ids, K, f, path="walk", sync=False), a.window_ms, a.repeats)
                        keep = mask
                    for per in PERS:
                        call = lambda lb=labels: m.compute_sub_topk_capped(ids, K, lb, per=per, filt=f, sync=False)
                        cell = dict(score=score, rows=n, labels=name, per=per, pred=f is not None, topk=t_topk)
                        cell["capped"] = windows(call, a.window_ms, a.repeats)
                        cell["splits"] = m.ctx.last_plan("capped_splits")
                        m.ctx.timing(True)
                        for _ in range(3):
                            call()
                        torch.cuda.synchronize()
                        for key in ("capped_walk", "capped_merge"):
                            ms, cnt = m.ctx.timing_get(key)
                            cell[key.replace("capped_", "") + "_us"] = round(1e3 * ms / cnt, 2) if cnt else None
                        m.ctx.timing(False)
                        fused = call()
                        cell["filled"] = round(float((fused >= 0).sum(dim=1).float().mean()), 2)
                        if name == "five":                                            # the gate without the fill table: PoiLabels of another filter
                            other = built[filt if f is None else None]
                            cell["nofill"] = windows(lambda: call(other), a.window_ms, a.repeats)
                            assert torch.equal(call(other), fused)
                        if f is None:
                            cell["cand"] = windows(lambda: greedy(cand(), labels.labels, per, K), a.window_ms, a.repeats)
                            cell["short"] = round(float((greedy(cand(), labels.labels, per, K) != fused).any(dim=1).float().mean()), 4)
                        if n <= 64 or (name == "zipf" and per == 2):                  # (thousands of rows: one labelling and cap - the sort alone takes long)

                            def matrix():
                                full = m.compute_sub_all_scores_device(ids)
                                if keep is not None:
                                    full = full.masked_fill(~keep, float("-inf"))
                                v, order = torch.sort(full, dim=1, descending=True, stable=True)
                                return greedy(torch.where(torch.isneginf(v), torch.full_like(order, -1), order).int(), labels.labels, per, K)
                            cell["matrix"] = windows(matrix, a.window_ms, a.repeats)
                            cell["same_ids"] = round(float((matrix() == fused).all(dim=1).float().mean()), 4)
                        print("[bench_capped] %s rows %d %s per %d pred %s: capped %.1f (walk %s merge %s) nofill %s | topk %.1f cand %s (short %s) matrix %s us"
                              % (score, n, name, per, f is not None, cell["capped"]["us"], cell["walk_us"], cell["merge_us"], cell.get("nofill", {}).get("us"),
                                 t_topk["us"], cell.get("cand", {}).get("us"), cell.get("short"), cell.get("matrix", {}).get("us")), file=sys.stderr, flush=True)
                        out["cells"].append(cell)
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
