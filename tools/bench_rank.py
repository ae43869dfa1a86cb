#!/usr/bin/env python
"""Exact target ranks (models.compute_sub_target_rank, poi_score_rank) at the Gowalla shape (N = 100 k POIs): the rank of every row's
held-out POI among all POIs, for dim 64 / 128, the plain score (BPR tables) and the spatial score (bins on the fly), launches of
64 / 4096 / 50 000 rows - beside compute_sub_topk(k = 20) over the same rows in the same process (unseeded: every call pays its full
price): existing code that forms the same product with a heavier epilogue, the yardstick.
Per cell: microseconds per call as the median of --repeats timed windows of at least --window-ms each (min and max alongside) of
chained calls with ONE synchronisation at the end of the window, after a warm-up window; the ratio rank / topk of the medians; the
item split the rank call took.  Device tensors go in, so no upload is timed.  Prints one JSON line.
    python tools/bench_rank.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness


def windows(fn, window_ms, repeats):
    def one():
        calls, t0 = 0, time.perf_counter()
        while True:
            fn()
            calls += 1
            if (time.perf_counter() - t0) * 1e3 >= window_ms:
                break
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, K = (4096, 10000, 20) if a.quick else (50000, 100000, 20)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, k=K), cells=[])
    rng = np.random.default_rng(3)
    for D in (64, 128):
        for spatial in (False, True):
            p = harness.default_params()
            p.update(latent_size=D, gru=2 if spatial else 0)
            m = harness.build_model(ds, p, seed=5)
            m.update_trained_items()
            if spatial:
                m.update_trained_dists()
                m.update_trained_users(torch.rand((U, D), device=m.device) - 0.5)
                m.update_trained_sus(torch.rand((U, m.n_dist + 1), device=m.device))
                m.use_bin_matrix = False                      # top-K with the bins on the fly too: the same distance term, the same way
            else:
                m.update_trained_users()
            m.topk_seeding = False
            for n in (64, 4096, U):
                if n > U:
                    continue
                rows = np.arange(n, dtype=np.int32) if n == U else torch.as_tensor(np.sort(rng.permutation(U)[:n]).astype(np.int32)).to(m.device)
                rank = windows(lambda: m.compute_sub_target_rank(rows, sync=False), a.window_ms, a.repeats)
                splits = m.ctx.last_plan("rank_splits")
                topk = windows(lambda: m.compute_sub_topk(rows, K), a.window_ms, a.repeats)
                out["cells"].append(dict(dim=D, score="geo" if spatial else "plain", rows=n, rank=rank, topk=topk, rank_splits=splits,
                                         ratio=round(rank["us"] / topk["us"], 3)))
            assert m.ctx.take_bad_ids() == 0
            del m
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
