#!/usr/bin/env python
"""Restricted recommendation (models.compute_sub_topk_near, poi_score_topk_near) at the Gowalla shape (N = 100 k POIs in a ~40 km box,
dim 128, BPR tables): top-20 within 1 / 5 / 20 km of the user's last train POI for launches of 1 / 64 / 4096 rows, beside
    (a) dense       compute_sub_topk over ALL POIs for the same rows (the fused tile kernels; answers another question - no radius),
    (b) torch       a torch-ops yardstick of the same restricted answer: dense scores (users @ items^T), a float64 Haversine mask
                    from the coordinates, torch.topk.
Per cell: microseconds per call as the median of --repeats timed windows of at least --window-ms each (min and max alongside) of
chained calls with ONE synchronisation at the end of the window, after a warm-up window; us per row and rows/s follow from the median.
Device tensors go in, so no upload is timed.  Also the mean candidate count per radius and the plan of every launch size.
Prints one JSON line.
    python tools/bench_near.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness


def windows(fn, window_ms, repeats):
    def one():
        calls, t0 = 0, time.perf_counter()
        while True:
            for _ in range(4):
                fn()
            calls += 4
            if (time.perf_counter() - t0) * 1e3 >= window_ms:
                break
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def per_row(r, n):
    r["us_per_row"] = round(r["us"] / n, 3)
    r["rows_per_s"] = round(n / r["us"] * 1e6)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="2 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, D, K = (2048, 10000, 128, 20) if a.quick else (8192, 100000, 128, 20)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 50, seed=1, dd=200, ud_km=40, local=0.8)
    p = harness.default_params()
    p.update(latent_size=D, gru=0)
    m = harness.build_model(ds, p, seed=5)
    m.update_trained_items(); m.update_trained_users()
    m.set_coords(ds.coords)
    m.topk_seeding = False                                   # every dense call pays its full price
    xy, cphi = m.coords, m._cphi
    items = m.trained_items.t[:N]
    last = m._last_train_poi()
    out = dict(shape=dict(users=U, pois=N, dim=D, k=K), radii={}, dense={}, plan={})
    rng = np.random.default_rng(3)
    sets = {n: torch.as_tensor(np.sort(rng.permutation(U)[:n]).astype(np.int32)).to(m.device) for n in (1, 64, min(4096, U))}
    for n, rows in sets.items():
        out["dense"][str(n)] = per_row(windows(lambda: m.compute_sub_topk(rows, K), a.window_ms, a.repeats), n)
    for r_km in (1.0, 5.0, 20.0):
        c_r = m._near_radius(r_km)
        res = {}
        for n, rows in sets.items():
            cnt = m.compute_sub_topk_near(rows, K, within_km=r_km, return_counts=True)[1]
            cell = dict(candidates_mean=round(float(cnt.float().mean().item()), 1))
            cell["near"] = per_row(windows(lambda: m.compute_sub_topk_near(rows, K, within_km=r_km, sync=False), a.window_ms, a.repeats), n)
            out["plan"][str(n)] = dict(path=m.ctx.last_plan("near_path"), splits=m.ctx.last_plan("near_splits"))
            anc = last.index_select(0, rows.long()).long()

            def torch_ops():
                sc = m.trained_users.t.index_select(0, rows.long()) @ items.T
                la = (xy[anc, 0][:, None] - xy[None, :, 0]) * 0.017453292519943295
                lo = (xy[anc, 1][:, None] - xy[None, :, 1]) * 0.017453292519943295
                c = (1.0 - torch.cos(la)) / 2 + cphi[anc][:, None] * cphi[None, :] * (1.0 - torch.cos(lo)) / 2
                return torch.topk(sc.masked_fill(~(c < c_r), float("-inf")), K, dim=1)
            if n <= 64 or not a.quick:
                cell["torch"] = per_row(windows(torch_ops, a.window_ms, max(3, a.repeats // 2)), n)
            res[str(n)] = cell
        out["radii"]["%g" % r_km] = res
    assert m.ctx.take_bad_ids() == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
