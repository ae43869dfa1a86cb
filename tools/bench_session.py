#!/usr/bin/env python
"""Online sessions (models.Session, poi_session_advance) at the Gowalla shape (U = 50 k users, N = 100 k POIs, B = 200 bins, L <= 50) for
D = 20, 64, 128: what ONE more check-in costs, against the only way to get the same answer without a session - rerunning the forward
pass over the users' whole training rows (`predict_device`), then ranking (`compute_sub_topk` / the geo top-K on those rows).
Per dim:
    advance               n = 1, 64, 4096, 50 000 events (distinct slots), beside predict_device over the same n users
    advance + recommend   n = 1, 64 (top-20), beside predict_device + top-20 over the same users
    forced paths          the event and the tile kernel on the other side of the switch point (option "session_tile_min")
Every figure is the median of --repeats timed windows of about --window-ms each (min and max alongside) of chained calls with ONE
synchronisation at the end of the window, after a calibration and a warm-up window; device tensors go in, so no upload is timed.  Prints one JSON line.
The baselines Lstm, Rnn and CA-RNN (models.CellSession, poi_session_cell_advance / poi_session_carnn_advance) get the same `advance`
and forced-path figures beside their own `predict_device` over the same users, under "cells" (dims that are no multiple of 16 have no
tile path: their forced figures are both the event kernel, and say so in "path").
    python tools/bench_session.py [--dims 20,64,128] [--models gru,lstm,rnn,carnn] [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness


def windows(fn, window_ms, repeats):
    """Median / min / max microseconds per call over `repeats` windows of about window_ms, after one warm-up window.  A window is a
    fixed number of chained calls with one synchronisation at its end; the number comes from a synchronised calibration of four calls,
    so the host never queues more than about one window of device work ahead (launches return long before a large call finishes)."""
    def run(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    run(4)
    calls = int(min(max(4, window_ms * 1e3 / max(run(4), 1e-3)), 100000))
    run(calls)
    v = sorted(run(calls) for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2), calls=calls)


def note(msg):
    print("[bench_session] " + msg, file=sys.stderr, flush=True)


def bench_cells(ds, p, a, kinds, dims, rng):
    """advance at n = 1 / 64 / 4096 / U and both kernels forced across the switch, beside predict_device, for Lstm / Rnn / CA-RNN."""
    from poi_amd import models
    U, N = ds.n_user, ds.n_item
    out = {}
    for kind in kinds:
        out[kind] = {}
        for D in dims:
            if kind == "carnn":
                m = harness.build_model(ds, dict(p, latent_size=D, gru=3), seed=5)
                m.update_trained_dists()
            else:
                m = getattr(models, harness.MINIBATCH_CELLS[kind])(train=ds.shard(), test=None, alpha_lambda=[p["alpha"], p["lambda"]], n_user=U, n_item=N,
                                                                   n_in=D, n_hidden=D, seed=5)
            m.update_trained_items()
            s = m.cell_session()
            s.load_history()
            res = dict(tile_min=None, advance={}, forced={})
            for n in (1, 64, 4096, U):
                n = min(n, U)
                users = np.sort(rng.permutation(U)[:n])
                sl = torch.as_tensor(users.astype(np.int32)).to(m.device)
                po = torch.as_tensor(rng.integers(0, N, n).astype(np.int32)).to(m.device)
                r = dict(advance=windows(lambda: s.advance(sl, po, sync=False), a.window_ms, a.repeats))
                r["path"] = m.ctx.last_plan("session_path")
                res["tile_min"] = m.ctx.last_plan("session_tile_min")
                r["predict"] = windows(lambda: m.predict_device(sl), a.window_ms, a.repeats)
                res["advance"][str(n)] = r
                if n in (64, 4096):
                    for name, tm in (("event", 1 << 30), ("tile", 1)):
                        m.ctx.set_option("session_tile_min", tm)
                        try:
                            f = windows(lambda: s.advance(sl, po, sync=False), a.window_ms, a.repeats)
                            f["path"] = m.ctx.last_plan("session_path")
                            res["forced"]["%s@%d" % (name, n)] = f
                        finally:
                            m.ctx.set_option("session_tile_min", res["tile_min"])
            assert m.ctx.take_bad_ids() == 0
            out[kind][str(D)] = res
            note("%s dim %d: %s" % (kind, D, json.dumps(res)))
            del s, m
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="20,64,128")
    ap.add_argument("--models", default="gru,lstm,rnn,carnn", help="gru = the GRU-family figures; lstm / rnn / carnn = the CellSession figures")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="5 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N = (5000, 10000) if a.quick else (50000, 100000)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 50, seed=1, dd=200, ud_km=40, local=0.8)
    note("data set built: %d users, %d POIs" % (U, N))
    p = harness.default_params()
    out = dict(shape=dict(users=U, pois=N, bins=ds.dist_num, mean_len=float(np.diff(ds.off).mean())), dims={})
    rng = np.random.default_rng(3)
    which = [x for x in a.models.split(",") if x]
    dims = [int(x) for x in a.dims.split(",")]
    for D in dims if "gru" in which else []:
        p.update(latent_size=D, gru=2)
        m = harness.build_model(ds, p, seed=5)
        m.update_trained_items(); m.update_trained_dists()
        hts, sts = m.predict_device(np.arange(U))
        m.update_trained_users(hts); m.update_trained_sus(sts)
        s = m.session()
        s.load_history()
        res = dict(kdim=m.kdim, tile_min=None, advance={}, recommend={}, forced={})
        for n in (1, 64, 4096, U):
            n = min(n, U)
            users = np.sort(rng.permutation(U)[:n])
            sl = torch.as_tensor(users.astype(np.int32)).to(m.device)
            po = torch.as_tensor(rng.integers(0, N, n).astype(np.int32)).to(m.device)
            r = dict(advance=windows(lambda: s.advance(sl, po, sync=False), a.window_ms, a.repeats))
            r["path"] = m.ctx.last_plan("session_path")
            res["tile_min"] = m.ctx.last_plan("session_tile_min")
            r["predict"] = windows(lambda: m.predict_device(sl), a.window_ms, a.repeats)
            res["advance"][str(n)] = r
            if n <= 64:
                q = dict(session=windows(lambda: (s.advance(sl, po, sync=False), s.recommend(sl, 20)), a.window_ms, a.repeats))

                def parent():
                    h, t = m.predict_device(sl)
                    m.trained_users.t[sl.long()] = h
                    t[:, m.n_dist] = 0.0
                    m._sus_masked[sl.long()] = t
                    return m.compute_sub_topk(sl, 20)
                q["predict_then_rank"] = windows(parent, a.window_ms, a.repeats)
                res["recommend"][str(n)] = q
            if n in (64, 4096):
                for name, tm in (("event", 1 << 30), ("tile", 1)):
                    m.ctx.set_option("session_tile_min", tm)
                    try:
                        res["forced"]["%s@%d" % (name, n)] = windows(lambda: s.advance(sl, po, sync=False), a.window_ms, a.repeats)
                    finally:
                        m.ctx.set_option("session_tile_min", res["tile_min"])
        assert m.ctx.take_bad_ids() == 0
        out["dims"][str(D)] = res
        note("gru dim %d: %s" % (D, json.dumps(res)))
        del s, m
        torch.cuda.empty_cache()
    cells = [k for k in ("lstm", "rnn", "carnn") if k in which]
    if cells:
        out["cells"] = bench_cells(ds, p, a, cells, dims, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
