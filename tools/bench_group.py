#!/usr/bin/env python
"""Group recommendation (models.recommend_group, poi_group_topk) at the Gowalla shape (N = 100 k POIs, dim 128): the top-20 of the mean
and of the minimum of the members' scores, the plain score (BPR tables) and the spatial score (bins on the fly), for 1 / 64 / 4096
groups of 4 members and 64 groups of 16 and of 64 members - beside the MATRIX ROUTE over the same groups in the same process, the
yardstick: the members' float32 score rows (compute_sub_all_scores_device, whole groups within 2 GiB at a time), torch mean / amin over
the members and torch.topk.
Per cell: microseconds per call as the median of --repeats timed windows of at least --window-ms each (min and max alongside) of
chained calls with ONE synchronisation at the end of the window, after a warm-up window; the ratio fused / matrix of the medians; the
plan the fused call took.  Host group lists go in, so their check and the gather of the members' rows are timed.  Prints one JSON line.
    python tools/bench_group.py [--repeats N] [--window-ms T] [--quick]"""
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


def matrix_route(m, ids, n_grp, M, agg, k):
    """The yardstick: score rows of every member, the aggregate over the members, torch.topk - whole groups within 2 GiB of rows."""
    step = max(1, (1 << 29) // (M * m.n_item))
    out = []
    for g in range(0, n_grp, step):
        c = min(step, n_grp - g)
        full = m.compute_sub_all_scores_device(ids[g * M:(g + c) * M]).view(c, M, m.n_item)
        a = full.mean(dim=1) if agg == "mean" else full.amin(dim=1)
        out.append(torch.topk(a, k, dim=1).indices)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, K, D = (4096, 10000, 20, 128) if a.quick else (50000, 100000, 20, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, k=K, dim=D), cells=[])
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
        for n_grp, M in ((1, 4), (64, 4), (4096, 4), (64, 16), (64, 64)):
            ids = rng.integers(0, U, n_grp * M)
            off = np.arange(n_grp + 1) * M
            ids_t = torch.as_tensor(ids.astype(np.int32)).to(m.device)
            for agg in ("mean", "min"):
                fused = windows(lambda: m.recommend_group((off, ids), K, agg=agg, sync=False), a.window_ms, a.repeats)
                plan = {k: m.ctx.last_plan(k) for k in ("group_path", "group_splits")}
                matrix = windows(lambda: matrix_route(m, ids_t, n_grp, M, agg, K), a.window_ms, a.repeats)
                out["cells"].append(dict(score="geo" if spatial else "plain", groups=n_grp, members=M, agg=agg, fused=fused, matrix=matrix, plan=plan,
                                         ratio=round(fused["us"] / matrix["us"], 3)))
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
