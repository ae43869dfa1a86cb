#!/usr/bin/env python
"""Route recommendation (Session.recommend_route: poi_route_expand + poi_route_merge + the session advance) at the Gowalla shape
(N = 100 k POIs, dim 128, 200 bins): the best `beam` routes of `steps` next POIs for 1 / 64 / 4096 slots, beam 4 and 8, 4 and 8 steps,
under the spatial score (OboSpatialGru, bins on the fly) and the plain one (OboGru) - beside the MATRIX ROUTE in the same process, the
yardstick: the same beam search through the (rows, n_item) float32 score matrix (poi_score_all [+ poi_dist_prob], at most 1 GiB of rows
at a time), torch.logsumexp in float64, a -inf mask over the last POI and the path, torch.topk per row and per slot, and the same
scratch session advance.
Per cell: microseconds per call as the median of --repeats timed windows of about --window-ms each (min and max alongside) of chained
calls with ONE synchronisation at the end of the window, after a calibration and a warm-up window; the ratio fused / matrix of the
medians; the plan the fused call's last expand took; and - from a separate pass under the library's event timing - the microseconds
one fused call spends in the expand, merge and advance kernels.  Device slot ids go in.  Prints one JSON line.
    python tools/bench_route.py [--repeats N] [--window-ms T] [--slots 1,64,4096] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness
from poi_amd.models import _ptr


def windows(fn, window_ms, repeats):
    """Median / min / max microseconds per call over `repeats` windows of about window_ms, after one warm-up window.  A window is a
    fixed number of chained calls with one synchronisation at its end; the number comes from a synchronised calibration."""
    def run(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    run(1)
    calls = int(min(max(1, window_ms * 1e3 / max(run(2), 1e-3)), 100000))
    run(calls)
    v = sorted(run(calls) for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2), calls=calls)


def note(msg):
    print("[bench_route] " + msg, file=sys.stderr, flush=True)


def score_rows(s, users, sts, lp):
    """(c, n_item) float32 scores of explicit rows: poi_score_all, plus poi_dist_prob's term for the spatial model."""
    m = s.m
    c = users.shape[0]
    prob = wd = None
    if s.spatial:
        st = (sts * (lp >= 0).float()[:, None]).contiguous()
        st[:, m.n_dist] = 0.0
        prob = torch.empty((c, m.n_item), dtype=torch.float32, device=m.device)
        m.ctx.check(m.lib.poi_dist_prob(m.ctx.handle, _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), _ptr(lp.clamp(min=0).contiguous()), _ptr(st), c,
                                        m.n_item, m.n_dist, m.dd * 1000.0, _ptr(prob), m._stream()))
        wd = m.wd.t
    full = torch.empty((c, m.n_item), dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_score_all(m.ctx.handle, _ptr(users), _ptr(m.trained_items.t), c, m.n_item, m.kdim, _ptr(wd), _ptr(prob), _ptr(full), m._stream()))
    return full


def matrix_route(s, ids, T, B):
    """The yardstick: the same search through explicit score rows."""
    m = s.m
    n, N, dev = ids.numel(), m.n_item, m.device
    src = {k: getattr(s, k).index_select(0, ids) for k in ("h", "sts", "last_poi", "steps") if getattr(s, k, None) is not None}
    last = src["last_poi"].long()
    scratch = type(s)(m, n_slot=n * B)
    all_rows = torch.arange(n * B, dtype=torch.int32, device=dev)
    base = torch.arange(n, device=dev)[:, None]
    total = torch.zeros((n, 1), dtype=torch.float64, device=dev)
    paths = torch.full((n * B, T), -1, dtype=torch.int64, device=dev)
    P = 1
    step = max(1, (1 << 28) // N)
    for t in range(T):
        users = src["h"].float().contiguous()
        R = users.shape[0]
        cs = torch.empty((R, B), dtype=torch.float32, device=dev)
        ci = torch.empty((R, B), dtype=torch.int64, device=dev)
        lse = torch.empty(R, dtype=torch.float64, device=dev)
        for o in range(0, R, step):
            c = min(step, R - o)
            full = score_rows(s, users[o:o + c], src["sts"][o:o + c] if s.spatial else None, src["last_poi"][o:o + c] if s.spatial else None)
            lse[o:o + c] = torch.logsumexp(full.double(), 1)
            lastp = last[torch.arange(o, o + c, device=dev) // P]
            full.scatter_(1, lastp.clamp(min=0)[:, None], float("-inf"))      # (every slot of the benchmark has a last POI)
            if t > 0:
                full.scatter_(1, paths[o:o + c, :t], float("-inf"))
            cs[o:o + c], ci[o:o + c] = torch.topk(full, B, dim=1)
        prop = total.reshape(n, P, 1) + (cs.double() - lse[:, None]).reshape(n, P, B)
        total, ti = torch.topk(prop.reshape(n, P * B), B, dim=1)
        poi = ci.reshape(n, P * B).gather(1, ti)
        flat = (base * P + ti // B).reshape(-1)
        if t > 0:
            paths = paths.index_select(0, flat)
        paths[:, t] = poi.reshape(-1)
        if t + 1 == T:
            break
        for k in src:
            setattr(scratch, k, src[k].index_select(0, flat).contiguous())
        nxt = poi.reshape(-1).int().contiguous()
        scratch._launch(all_rows.data_ptr(), nxt.data_ptr(), n * B)
        src = {k: getattr(scratch, k) for k in src}
        P = B
    return paths.view(n, B, T), total


def kernel_times(m, fn, calls=3):
    """Microseconds per call in the expand / merge / advance kernels, from the library's event timing."""
    m.ctx.timing(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in ("route_expand", "route_merge", "session_advance"):
        ms, cnt = m.ctx.timing_get(name)
        out[name] = dict(us=round(ms * 1e3 / calls, 2), launches=cnt // calls)
    m.ctx.timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--slots", default="1,64,4096")
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (8192, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    note("data set built: %d users, %d POIs, %d bins" % (U, N, ds.dist_num))
    out = dict(shape=dict(users=U, pois=N, dim=D, bins=ds.dist_num), cells=[])
    rng = np.random.default_rng(3)
    for spatial in (True, False):
        p = harness.default_params()
        p.update(latent_size=D, gru=2 if spatial else 1)
        m = harness.build_model(ds, p, seed=5)
        m.update_trained_items()
        if spatial:
            m.update_trained_dists()
        s = m.session()
        s.load_history()
        for n in [int(x) for x in a.slots.split(",")]:
            n = min(n, U)
            ids = torch.as_tensor(np.sort(rng.permutation(U)[:n])).to(m.device)
            for B in (4, 8):
                for T in (4, 8):
                    fused = windows(lambda: s.recommend_route(ids, T, beam=B, sync=False), a.window_ms, a.repeats)
                    plan = {k: m.ctx.last_plan(k) for k in ("route_path", "route_splits")}
                    kern = kernel_times(m, lambda: s.recommend_route(ids, T, beam=B, sync=False))
                    matrix = windows(lambda: matrix_route(s, ids, T, B), a.window_ms, a.repeats)
                    cell = dict(score="geo" if spatial else "plain", slots=n, beam=B, steps=T, fused=fused, matrix=matrix, kernels=kern, plan=plan,
                                ratio=round(fused["us"] / matrix["us"], 3))
                    note(json.dumps(cell))
                    out["cells"].append(cell)
        assert m.ctx.take_bad_ids() == 0
        del s, m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
