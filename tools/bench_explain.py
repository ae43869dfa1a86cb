#!/usr/bin/env python
"""Leave-one-out attribution (models.Explainer.explain, poi_explain_loo) at the Gowalla shape (N = 100 k POIs, D = 128, B = 200 bins,
L <= 50): C = 20 listed POIs, 1 / 64 / 4096 rows, the spatial and the plain model, both start modes (option "explain_start").
Per case:
    call        the whole explain() call, wall clock (groups and column tables included), median of --repeats timed calls after warm-up
    base, walk  the two launches on the device (timing names "explain_base" / "explain_walk"), per call, and microseconds per
                tile-step: a tile-step is one step of one 16-column workgroup; a launch costs sum over its tiles of the longest
                remaining walk
    session     the route that existed before, in the same process: a scratch Session of one slot per variant replayed through all
                reduced histories (built on the host beforehand, not timed) + score_lists; its scores must equal base - delta
Prints one JSON line.
    python tools/bench_explain.py [--rows 1,64,4096] [--models spatial,plain] [--repeats N] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness, models


def note(msg):
    print("[bench_explain] " + msg, file=sys.stderr, flush=True)


def median_us(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e6)
    v.sort()
    return dict(us=round(v[len(v) // 2], 1), min=round(v[0], 1), max=round(v[-1], 1))


def tile_steps(lens, g_off, first, row, mode):
    """(base, walk) tile-steps of a call: per 16-column tile of the column tables the longest remaining walk."""
    base, var = models.explain_columns(lens, g_off, first, row, mode)
    per_tile = lambda rem: int(sum(int(rem[i:i + 16].max()) for i in range(0, len(rem), 16)))
    lens = lens.cpu().numpy()
    b, v = base.cpu().numpy(), var.cpu().numpy()
    return per_tile(lens[b[:, 0]]), per_tile(lens[v[:, 0]] - v[:, 2]) if len(v) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,64,4096")
    ap.add_argument("--models", default="spatial,plain")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="5 k users / 10 k POIs, 3 repeats")
    a = ap.parse_args()
    U, N = (5000, 10000) if a.quick else (50000, 100000)
    if a.quick:
        a.repeats = 3
    ds = pdata.make_synthetic(U, N, 50, seed=1, dd=200, ud_km=40, local=0.8)
    note("data set built: %d users, %d POIs" % (U, N))
    p = harness.default_params()
    try:
        clock = torch.cuda.clock_rate()
    except Exception:
        clock = None
    out = dict(shape=dict(users=U, pois=N, bins=ds.dist_num, dim=a.dim, lists=a.lists, mean_len=float(np.diff(ds.off).mean())),
               device=torch.cuda.get_device_name(0), sclk_mhz=clock, repeats=a.repeats, cases={})
    rng = np.random.default_rng(3)
    for kind in [x for x in a.models.split(",") if x]:
        p.update(latent_size=a.dim, gru=2 if kind == "spatial" else 1)
        m = harness.build_model(ds, p, seed=5)
        m.update_trained_items()
        if kind == "spatial":
            m.update_trained_dists()
        ex = models.Explainer(m)
        p_all, off_all = m.p.cpu().numpy().astype(np.int64), m._off_host.astype(np.int64)
        for n in [min(int(x), U) for x in a.rows.split(",")]:
            users = np.sort(rng.permutation(U)[:n])
            lists = torch.as_tensor(rng.integers(0, N, (n, a.lists)).astype(np.int32)).to(m.device)
            seqs = [p_all[off_all[u]:off_all[u + 1]] for u in users]
            lens = np.array([len(s) for s in seqs])
            o = np.r_[0, np.cumsum(lens)]
            hist = (torch.as_tensor(o.astype(np.int32)).to(m.device), torch.as_tensor(np.concatenate(seqs).astype(np.int32)).to(m.device))
            grp, g_off, keys, first, row = models.explain_groups(hist[0].long(), hist[1], "checkin")
            res = dict(variants=int(g_off[-1]), mean_len=float(lens.mean()))
            got = {}
            for mode in (1, 0):
                m.ctx.set_option("explain_start", mode)
                call = lambda: ex.explain(users, lists, histories=hist, sync=False)
                r = dict(call=median_us(call, a.repeats))
                m.ctx.timing(True)
                for _ in range(a.repeats):
                    call()
                torch.cuda.synchronize()
                steps = tile_steps(torch.as_tensor(lens).to(m.device), g_off, first, row, mode)
                for name, ts in zip(("explain_base", "explain_walk"), steps):
                    ms, cnt = m.ctx.timing_get(name)
                    r[name[8:]] = dict(us=round(ms * 1e3 / max(cnt, 1), 1), tile_steps=ts, us_per_tile_step=round(ms * 1e3 / max(cnt, 1) / max(ts, 1), 3))
                m.ctx.timing(False)
                r["tiles"] = m.ctx.last_plan("explain_tiles")
                got[mode] = ex.explain(users, lists, histories=hist)
                res["start_%d" % mode] = r
            m.ctx.set_option("explain_start", 1)
            res["modes_bitwise_equal"] = bool(all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(got[1][:2], got[0][:2])))
            # the route that existed before: one session slot per variant, the reduced histories replayed, the lists scored
            G = int(g_off[-1])
            red_len = np.repeat(lens, lens) - 1
            r_off = np.r_[0, np.cumsum(red_len)]
            flat = np.concatenate(seqs)
            # variant g of row r holds the row's positions but its own: enumerate (variant, position) pairs and drop the diagonal
            v_row = np.repeat(np.arange(n), lens)
            pos = np.concatenate([np.tile(np.arange(L), L) for L in lens]) if G else np.zeros(0, np.int64)
            var = np.repeat(np.arange(G), np.repeat(lens, lens))
            own = var - np.repeat(o[:-1], lens * lens)
            keep = pos != own
            r_flat = flat[(np.repeat(o[:-1], lens * lens) + pos)[keep]]
            assert len(r_flat) == r_off[-1]
            s = m.session(max(G, 1))
            v_lists = lists[torch.as_tensor(v_row).to(m.device)]
            slots = torch.arange(G, device=m.device)

            def old():
                s.reset()
                s.replay(r_off, r_flat, sync=False)
                return s.score_lists(slots, v_lists, sync=False)
            res["session"] = median_us(old, max(3, a.repeats // 3), warm=1)
            sc = old().double()
            mine = (got[1][0][torch.as_tensor(v_row).to(m.device)] - got[1][1])
            res["max_rel_diff_to_session"] = float((mine - sc).abs().max() / sc.abs().max()) if G else 0.0
            note("%s rows %d: %s" % (kind, n, json.dumps(res)))
            out["cases"]["%s_%d" % (kind, n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
