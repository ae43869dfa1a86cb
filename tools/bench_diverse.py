#!/usr/bin/env python
"""Diversified recommendation (models.compute_sub_topk_diverse, poi_diverse_topk) at the Gowalla shape (N = 100 k POIs, dim 128): the
top-20 of a pool of 64, re-ranked by MMR (trade 0.7, scale 1 km) under the geo, the embedding and the mixed similarity, the plain score
(BPR tables) and the spatial score (bins on the fly), for calls of 1 / 64 / 4096 rows.  Beside it, in the same process:
  topk     compute_sub_topk(k = 20) over the same rows: what diversity costs over a plain list;
  matrix   the same definition through the score matrix: compute_sub_all_scores_device, torch.topk(64) and a batched float64 torch loop
           over the 20 steps (rows within 2 GiB of scores at a time);
  pool / rerank   the two stages alone (poi_diverse_pool, poi_diverse_rerank on that pool).
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls -
as many as fill --window-ms - with ONE synchronisation at the end of the window, after a warm-up window; the ratio fused / matrix of the medians; the
plan the pool took; the share of rows on which the matrix route picks the same list.  Then what the feature does to the lists: mean
intra-list distance (km) and catalogue coverage at trade 1.0 / 0.7 / 0.3 over 4096 rows.  Prints one JSON line.
    python tools/bench_diverse.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, evaluate, harness
from poi_amd.models import _ptr

POOL, SCALE = 64, 1.0
SIMS = (("geo", 1.0), ("embed", 0.0), ("mixed", 0.5))


def windows(fn, window_ms, repeats):
    """A window is a FIXED number of chained calls and one synchronisation: the number that fills window_ms at the duration of one
    synchronised call.  (Chaining until the host clock says so queues seconds of device work behind a raw library call that takes
    microseconds to enqueue.)"""
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


def torch_rerank(pi, ps, items, coords, cphi, k, trade, g, scale):
    """The re-ranking of include/poi_hip.h as batched float64 torch ops, one step at a time."""
    n, P = pi.shape
    p = pi.long()
    s = ps.double()
    den = s[:, :1] - s[:, -1:]
    rel = torch.where(den == 0, torch.ones_like(s), (s - s[:, -1:]) / torch.where(den == 0, torch.ones_like(den), den))
    if g > 0:
        lat, lon, cp = coords[p, 0], coords[p, 1], cphi[p]
    if g < 1:
        x = items[p].double()
        nrm = x.pow(2).sum(-1).sqrt()
    ar = torch.arange(n, device=pi.device)
    pen = torch.zeros_like(s)
    taken = torch.zeros_like(p, dtype=torch.bool)
    win = torch.zeros(n, dtype=torch.long, device=pi.device)
    picks = []
    for t in range(k):
        if t > 0:
            obj = trade * rel - (1.0 - trade) * pen
            win = obj.masked_fill(taken, float("-inf")).argmax(dim=1)
        picks.append(p[ar, win])
        taken[ar, win] = True
        if trade != 1.0 and t + 1 < k:
            sim = torch.zeros_like(s)
            if g > 0:
                sa = torch.sin((lat - lat[ar, win][:, None]) * (np.pi / 360.0)); sb = torch.sin((lon - lon[ar, win][:, None]) * (np.pi / 360.0))
                d = 12742.0 * torch.asin(torch.sqrt(sa * sa + cp * cp[ar, win][:, None] * sb * sb).clamp(max=1.0))
                sim = g * torch.exp(-d / scale)
            if g < 1:
                sim = sim + (1.0 - g) * (x * x[ar, win][:, None, :]).sum(-1) / (nrm * nrm[ar, win][:, None])
            pen = sim if t == 0 else torch.maximum(pen, sim)
    return torch.stack(picks, 1).int()


def matrix_route(m, ids, k, trade, g):
    step = max(1, (1 << 29) // m.n_item)
    out = []
    for o in range(0, len(ids), step):
        full = m.compute_sub_all_scores_device(ids[o:o + step])
        ps, pi = torch.topk(full, POOL, dim=1)
        out.append(torch_rerank(pi, ps, m.trained_items.t[:m.n_item], m.coords, m._cphi, k, trade, g, SCALE))
    return torch.cat(out)


def stages(m, ids):
    """(pool call, re-rank call factory) on the model's own rows: the two entries alone."""
    uid, users, lo = m._users_rows(ids)
    users, n, term = users.contiguous(), len(ids), m._rank_term(uid, lo)
    wd = sts = lp = coords = cphi = thr = None
    n_dist, dd_m = 0, 0.0
    if term is not None:
        wd, sts, lp = term
        coords, cphi, thr, n_dist, dd_m = m.coords, m._cphi, m._binthr, m.n_dist, m.dd * 1000.0
    items = m.trained_items.t
    pi = torch.empty((n, POOL), dtype=torch.int32, device=m.device)
    ps = torch.empty((n, POOL), dtype=torch.float32, device=m.device)
    out = torch.empty((n, 20), dtype=torch.int32, device=m.device)

    def pool():
        m.ctx.check(m.lib.poi_diverse_pool(m.ctx.handle, _ptr(users), _ptr(items), n, m.n_item, m.kdim, _ptr(wd), _ptr(sts), _ptr(coords), _ptr(cphi),
                                           _ptr(thr), _ptr(lp), int(n_dist), float(dd_m), None, None, POOL, _ptr(pi), _ptr(ps), None, m._stream()))

    def rerank(k, trade, g):
        return lambda: m.ctx.check(m.lib.poi_diverse_rerank(m.ctx.handle, _ptr(pi), _ptr(ps), n, POOL, _ptr(items) if g < 1 else None, m.n_item, m.kdim,
                                                            _ptr(m.coords) if g > 0 else None, _ptr(m._cphi) if g > 0 else None, k, trade, g, SCALE,
                                                            _ptr(out), None, None, None, m._stream()))
    return pool, rerank


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
    out = dict(shape=dict(users=U, pois=N, k=K, pool=POOL, dim=D, trade=0.7, scale_km=SCALE), cells=[], lists=[])
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
        for n in (1, 64, 4096):
            ids = rng.choice(U, n, replace=False).astype(np.int64)
            pool, rerank = stages(m, ids)
            t_topk = windows(lambda: m.compute_sub_topk(ids, K), a.window_ms, a.repeats)
            t_pool = windows(pool, a.window_ms, a.repeats)
            plan = {k: m.ctx.last_plan(k) for k in ("diverse_path", "diverse_splits")}
            for sim, g in SIMS:
                fused = windows(lambda: m.compute_sub_topk_diverse(ids, K, pool=POOL, trade=0.7, geo_weight=g, scale_km=SCALE, sync=False), a.window_ms, a.repeats)
                t_rr = windows(rerank(K, 0.7, g), a.window_ms, a.repeats)
                matrix = windows(lambda: matrix_route(m, ids, K, 0.7, g), a.window_ms, a.repeats)
                agree = float((m.compute_sub_topk_diverse(ids, K, pool=POOL, trade=0.7, geo_weight=g, scale_km=SCALE) == matrix_route(m, ids, K, 0.7, g))
                              .all(dim=1).float().mean())
                print("[bench_diverse] %s rows %d %s: fused %.1f us, matrix %.1f us" % (score, n, sim, fused["us"], matrix["us"]), file=sys.stderr, flush=True)
                out["cells"].append(dict(score=score, rows=n, sim=sim, fused=fused, pool=t_pool, rerank=t_rr, topk=t_topk, matrix=matrix, plan=plan,
                                         ratio=round(fused["us"] / matrix["us"], 3), over_topk=round(fused["us"] / t_topk["us"], 3), same_lists=round(agree, 4)))
        ids = np.arange(4096, dtype=np.int64)
        xy = m.coords.cpu().numpy()
        for sim, g in SIMS:
            for trade in (1.0, 0.7, 0.3):
                idx = m.compute_sub_topk_diverse(ids, K, pool=POOL, trade=trade, geo_weight=g, scale_km=SCALE).cpu().numpy()
                out["lists"].append(dict(score=score, sim=sim, trade=trade, intra_list_km=round(float(np.nanmean(evaluate.intra_list_distance_km(idx, xy))), 3),
                                         coverage=round(evaluate.catalogue_coverage(idx, N), 4)))
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
