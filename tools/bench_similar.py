#!/usr/bin/env python
"""Similar POIs (models.similar_pois, poi_similar_topk / poi_similar_rows) at the Gowalla shape (100 k POIs, 50 k users, dim 128): the
top-20 and the top-1000 similar POIs of 1 / 32 / 1024 / 100 k (all) query POIs under the cosine alone (g = 0) and the mixed similarity
(g = 0.5, scale 2 km); for k = 20 the fused walk ("similar_rows_max" 0) against the score rows + selection ("similar_rows_max" 4096),
each in the regime the planner gives it.  Beside it, in the same process:
  audience  poi_score_audience with the item table on both sides: the same walk by the raw dot product - what the similarity epilogue
            and the norms cost over it can be read off
  torch     normalize(items)[pois] @ normalize(items).T (queries within 1 GiB of scores at a time) + torch.topk, g = 0; the fused ids
            are checked against it where its float32 scores separate the neighbours in the list
  nearest   models.nearest_visited of 64 / 4096 rows with lists of 20 POIs over their train histories
--crossover: k = 20 for 1 .. 1024 queries on both routes - the table the "similar_rows_max" default is read from.
Per cell: microseconds per call as the median of --repeats timed windows of about --window-ms each (min and max alongside) of chained
calls with ONE synchronisation at the end of the window, after a warm-up window; then one call under the context's per-kernel event
timing (norms / walk / merge, or norms / rows / select) in microseconds.  Prints one JSON line on stdout; every finished cell goes to
stderr at once.
    python tools/bench_similar.py [--repeats N] [--window-ms T] [--quick] [--geo 0,0.5] [--queries 1,32,...] [--crossover] [--no-yardsticks] [--split-max N]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness

NAMES = ("similar_topk", "similar_norms", "similar_walk", "similar_merge", "similar_rows", "topk_select", "similar_nearest")


def windows(fn, window_ms, repeats):
    """The calls of a window are chained without a synchronisation, so their number is fixed beforehand from one synchronised call.  A
    call longer than the window is its own window (and its own warm-up)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    calls = max(1, min(100000, int(window_ms * 1e-3 / max(first, 1e-6))))

    def one():
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    if first <= window_ms * 1e-3:
        one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2), calls=calls)


def kernels(m, fn):
    """One call of fn under the per-kernel event timing -> {name: microseconds} of the names that ran."""
    m.ctx.timing(True)
    fn()
    torch.cuda.synchronize()
    out = {}
    for name in NAMES:
        ms, n = m.ctx.timing_get(name)
        if n:
            out[name] = round(ms * 1e3, 2)
    m.ctx.timing(False)
    return out


def torch_route(xn, q, k):
    """normalize(items)[pois] @ normalize(items).T + torch.topk (k + 1: the query itself is among them), within 1 GiB of scores at a time."""
    step = max(1, (1 << 28) // xn.shape[0])
    return torch.cat([torch.topk(xn[q[o:o + step].long()] @ xn.T, k + 1, dim=1).indices for o in range(0, q.numel(), step)])


def main():
    t_start = time.perf_counter()

    def emit(out, cell):
        out["cells"].append(cell)
        print("[%6.1f s] %s" % (time.perf_counter() - t_start, json.dumps(cell)), file=sys.stderr, flush=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    ap.add_argument("--geo", default="0,0.5", help="comma list of geo weights")
    ap.add_argument("--queries", default="", help="comma list of query counts (default 1,32,1024 and all POIs)")
    ap.add_argument("--crossover", action="store_true", help="k = 20 on both routes for 1 .. 1024 queries instead of the main table")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--split-max", type=int, default=-1, help='option "similar_split_max" for the run (default: the library\'s)')
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, dim=D), cells=[])
    rng = np.random.default_rng(3)
    p = harness.default_params()
    p.update(latent_size=D, gru=0)
    m = harness.build_model(ds, p, seed=5)
    m.update_trained_items()
    m.update_trained_users()
    if getattr(m, "coords", None) is None:
        m.set_coords(ds.coords)
    geos = [float(v) for v in a.geo.split(",") if v]
    counts = [int(v) for v in a.queries.split(",") if v] or ([1, 2, 4, 8, 16, 32, 64, 128, 256, 1024] if a.crossover else [1, 32, 1024, N])
    routes = (("fused", 0), ("rows", 4096))
    if a.split_max >= 0:
        m.ctx.set_option("similar_split_max", a.split_max)
        out["similar_split_max"] = a.split_max
    try:
        for n_q in counts:
            q = torch.as_tensor(rng.permutation(N)[:n_q].astype(np.int32)).to(m.device)
            for g in geos:
                for k in ((20,) if a.crossover else (20, 1000)):
                    for route, rows_max in (routes if k <= 32 else (("rows", 0),)):
                        if route == "rows" and k <= 32 and n_q > 4096:
                            continue
                        m.ctx.set_option("similar_rows_max", rows_max)
                        call = lambda: m.similar_pois(q, k, geo_weight=g, scale_km=2.0, sync=False)
                        cell = dict(g=g, queries=n_q, k=k, route=route, time=windows(call, a.window_ms, a.repeats))
                        cell["plan"] = {key: m.ctx.last_plan(key) for key in ("similar_path", "similar_splits")}
                        cell["kernels"] = kernels(m, call)
                        emit(out, cell)
            m.ctx.set_option("similar_rows_max", 1024)
            if a.no_yardsticks or a.crossover:
                continue
            x = m._items()
            rows = x[:N].float().contiguous()
            aud = lambda: m._audience_launch(rows, x, m.kdim, None, q, (None, None), 20, None, False, False, False)
            emit(out, dict(queries=n_q, k=20, route="audience", time=windows(aud, a.window_ms, a.repeats)))
            xn = torch.nn.functional.normalize(rows, dim=1)
            cell = dict(g=0.0, queries=n_q, k=20, route="torch", time=windows(lambda: torch_route(xn, q, 20), a.window_ms, a.repeats))
            if n_q <= 1024:                                   # same ids wherever the matrix route's own scores separate the neighbours
                got = m.similar_pois(q, 20).long()
                sc = xn[q.long()] @ xn.T
                sc[torch.arange(n_q, device=m.device), q.long()] = -2.0
                ref = torch.topk(sc, 21, dim=1)
                clear = (ref.values[:, :-1] - ref.values[:, 1:]).min(dim=1).values > 1e-5
                cell["same_ids"] = bool(torch.equal(got[clear], ref.indices[clear][:, :20]))
                cell["clear_queries"] = int(clear.sum().item())
            emit(out, cell)
        if not (a.no_yardsticks or a.crossover):
            for n in (64, 4096):
                n = min(n, U)
                rows = np.arange(n)
                lists = torch.as_tensor(rng.integers(0, N, (n, 20)).astype(np.int32)).to(m.device)
                for g in geos:
                    call = lambda: m.nearest_visited(rows, lists, geo_weight=g, scale_km=2.0, sync=False)
                    emit(out, dict(g=g, rows=n, k=20, route="nearest", time=windows(call, a.window_ms, a.repeats), kernels=kernels(m, call)))
    finally:
        m.ctx.set_option("similar_rows_max", 1024)
    assert m.ctx.take_bad_ids() == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
