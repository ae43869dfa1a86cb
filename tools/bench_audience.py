#!/usr/bin/env python
"""Audience recommendation (models.recommend_audience, poi_score_audience / poi_audience_rows) at the Gowalla shape (100 k POIs, 50 k
users, dim 128, 200 distance bins): the top-20 and the top-1000 USERS of 1 / 32 / 1024 / 100 k (all) query POIs, train visitors
excluded, under the plain score (BPR tables) and the spatial score (bins on the fly), in the split regime (slices of the user range)
and the block regime (one workgroup per 32-query block), each forced through "audience_split_max".  Host work that does not depend on
the call's scores (the visitor lists of the queries) is done once outside the windows.  Beside it, in the same process:
  torch    the matrix route on the PLAIN score: items[pois] @ users.T (queries within 1 GiB of scores at a time) + torch.topk; the
           fused ids are checked against it where the scores of neighbours in the list differ by more than a float32 rounding
  forward  the top-20 POIs of the SAME NUMBER OF ROWS (compute_sub_topk over that many users): the other direction's cost
Per cell: microseconds per call as the median of --repeats timed windows of about --window-ms each (min and max alongside) of
chained calls with ONE synchronisation at the end of the window, after a warm-up window; then one call under the context's per-kernel
event timing: walk / merge (k = 20) or rows / select (k = 1000) in microseconds.  Prints one JSON line on stdout; every finished cell
goes to stderr at once.
    python tools/bench_audience.py [--repeats N] [--window-ms T] [--quick] [--scores plain,geo] [--queries 1,32,...]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness


def windows(fn, window_ms, repeats):
    """The calls of a window are chained without a synchronisation, so their number is fixed beforehand from one synchronised call:
    enqueueing for window_ms of HOST time would queue seconds of work for the calls that take milliseconds on the device."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(1, min(100000, int(window_ms * 1e-3 / max(time.perf_counter() - t0, 1e-6))))

    def one():
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def kernels(m, fn, names):
    """One call of fn under the per-kernel event timing -> {name: microseconds} of the names that ran."""
    m.ctx.timing(True)
    fn()
    torch.cuda.synchronize()
    out = {}
    for name in names:
        ms, n = m.ctx.timing_get(name)
        if n:
            out[name] = round(ms * 1e3, 2)
    m.ctx.timing(False)
    return out


def torch_route(m, q, k):
    """items[pois] @ users.T + torch.topk, queries within 1 GiB of scores at a time (the plain score)."""
    items, users = m._items()[:m.n_item].float(), m.trained_users.t
    step = max(1, (1 << 28) // users.shape[0])
    return torch.cat([torch.topk(items[q[o:o + step].long()] @ users.T, k, dim=1).indices for o in range(0, q.numel(), step)])


def main():
    t_start = time.perf_counter()

    def emit(out, cell):
        """A finished cell: kept for the JSON line, and shown on stderr at once (the full shape runs for minutes)."""
        out["cells"].append(cell)
        print("[%6.1f s] %s" % (time.perf_counter() - t_start, json.dumps(cell)), file=sys.stderr, flush=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    ap.add_argument("--scores", default="plain,geo", help="comma list of plain / geo")
    ap.add_argument("--queries", default="", help="comma list of query counts (default 1,32,1024 and all POIs)")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, dim=D), cells=[])
    rng = np.random.default_rng(3)
    counts = [int(v) for v in a.queries.split(",") if v] or [1, 32, 1024, N]
    for spatial in (False, True):
        if ("geo" if spatial else "plain") not in a.scores.split(","):
            continue
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
        m.train_visitors()
        for n_q in counts:
            pois = rng.permutation(N)[:n_q].astype(np.int32)
            q = torch.as_tensor(pois).to(m.device)
            ex = m._audience_exclusion("train", q, None, U)   # the queries' visitor lists, gathered once: device lists go in as they are
            for k in (20, 1000):
                for regime, split_max in (("split", 1 << 30), ("block", 0)):
                    m.ctx.set_option("audience_split_max", split_max)
                    call = lambda: m.recommend_audience(q, k, exclude=ex, sync=False)
                    cell = dict(score="geo" if spatial else "plain", queries=n_q, k=k, regime=regime, fused=windows(call, a.window_ms, a.repeats))
                    cell["plan"] = {key: m.ctx.last_plan(key) for key in ("audience_path", "audience_splits")}
                    cell["kernels"] = kernels(m, call, ("score_audience", "audience_walk", "audience_merge", "audience_rows", "topk_select"))
                    emit(out, cell)
                m.ctx.set_option("audience_split_max", 256)
                if not spatial:
                    cell = dict(score="plain", queries=n_q, k=k, regime="torch", fused=windows(lambda: torch_route(m, q, k), a.window_ms, a.repeats))
                    if k == 20 and n_q <= 1024:               # same ids wherever the matrix route's own scores separate the neighbours
                        got = m.recommend_audience(q, k).long()
                        sc = m._items()[:N].float()[q.long()] @ m.trained_users.t.T
                        ref = torch.topk(sc, k + 1, dim=1)
                        clear = (ref.values[:, :-1] - ref.values[:, 1:]).min(dim=1).values > 1e-5 * sc.abs().max()
                        cell["same_ids"] = bool(torch.equal(got[clear], ref.indices[clear][:, :k]))
                        cell["clear_queries"] = int(clear.sum().item())
                    emit(out, cell)
            if n_q <= U:                                      # the forward direction on the same number of rows
                rows = np.arange(n_q)
                emit(out, dict(score="geo" if spatial else "plain", queries=n_q, k=20, regime="forward",
                               fused=windows(lambda: m.compute_sub_topk(rows, 20), a.window_ms, a.repeats)))
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
