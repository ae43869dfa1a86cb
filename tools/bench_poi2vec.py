#!/usr/bin/env python
"""POI2Vec step (poi_poi2vec_step, public/POI2Vec.py:127-177) at D = 20 and 64, one-user launches and launches of 64 users, on a synthetic
check-in set spread over a 1500 km box (make_poi2vec_synthetic, local = 0.8: a region tree of >= 4096 leaves).  Every figure is the
median of --repeats timed windows of at least --window-ms each (min and max alongside), after a warm-up window over the same launches.
Prints one JSON line: wall time per launch (host clock around chained launches: it includes train_batch's host work and the upload of
the user ids), the sum of the kernel times of a launch (HIP events), the bytes of wl read and written twice per launch (the dense
update's floor), a BATCHED torch-ops yardstick of the same rule (one autograd graph per launch: S = XU WL^T, log-softmax, the tree
terms of all positions at once, backward, the dense wl / xu / pb update; without the last-wins collapse, which only makes it cheaper),
and the top-20 of every user (poi_poi2vec_topk).
    python tools/bench_poi2vec.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness

KERNELS = ("p2v_plan", "p2v_lse", "p2v_pos", "p2v_user", "p2v_sort", "p2v_pb", "p2v_dense", "p2v_sparse", "p2v_xu")
SC_KERNELS = ("p2v_sc_node", "p2v_sc_route", "p2v_sc_plu", "p2v_sc_out", "p2v_sc_topk")


def torch_launch_data(m, users):
    """Host side of the yardstick, prepared once per launch outside the timed window: flat targets, padded contexts, owner of each position."""
    off, coff = m._tra[0].astype(np.int64), m._tra[2].astype(np.int64)
    t, own, inv, ctx = [], [], [], []
    for k, u in enumerate(users):
        L = int(off[u + 1] - off[u])
        t.extend(m._tra[1][off[u]:off[u + 1]].tolist()); own.extend([k] * L); inv.extend([1.0 / L] * L)
        ctx.extend(m._tra[3][coff[x]:coff[x + 1]] for x in range(off[u], off[u + 1]))
    cmax = max([len(c) for c in ctx] + [1])
    cidx = np.full((len(ctx), cmax), m.n_item, np.int64)
    for i, c in enumerate(ctx):
        cidx[i, :len(c)] = c
    dev = m.device
    T = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=dev)
    return dict(users=T(np.asarray(users, np.int64), torch.int64), t=T(t, torch.int64), own=T(own, torch.int64), inv=T(inv, torch.float32),
                cidx=T(cidx, torch.int64), k=len(users))


def torch_step(m, W, Ld, alpha=0.01, lam=0.001):
    """One launch with torch ops on the tables W (updated in place)."""
    wl, xu, pb = (W[k].detach().requires_grad_() for k in ("wl", "xu", "pb"))
    t = Ld["t"]
    x = xu[Ld["users"]]
    lp = torch.log_softmax(x @ wl[:m.n_item].T, 1)[Ld["own"], t]
    c = wl[Ld["cidx"]].sum(1)
    ind = torch.ceil(c.mean(1).abs()).detach()
    z = (pb[m.routes[t].long()] * c[:, None, None, :]).sum(3)
    br = torch.sigmoid(z * m.lrs[t].float()) * ind[:, None, None]
    S = (br.prod(2) * m.probs[t]).sum(1)
    paths = torch.floor(1 - S).detach() + S
    cost = -((lp + torch.log(paths)) * Ld["inv"]).sum() + 0.5 * lam * ((x ** 2).sum() + Ld["k"] * (wl ** 2).sum())
    cost.backward()
    with torch.no_grad():
        for k, v in (("wl", wl), ("xu", xu), ("pb", pb)):
            W[k] = v - alpha * v.grad
        W["wl"][-1] = 0                                         # the pad row wl_m never moves


def windows(fn, n_calls, window_ms, repeats):
    """Median / min / max of the time per call over `repeats` windows of >= window_ms, after one warm-up window."""
    def one(calls):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(calls):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    calls = max(n_calls, 8)
    dt = one(calls)                                             # warm-up, and sizes the window
    calls = max(calls, int(np.ceil(calls * window_ms * 1e-3 / max(dt, 1e-9))))
    per = sorted(one(calls) / calls for _ in range(repeats))
    return dict(median_ms=1e3 * per[len(per) // 2], min_ms=1e3 * per[0], max_ms=1e3 * per[-1], calls_per_window=calls, windows=repeats)


def run(dim, B, a):
    n_user, n_item = (600, 20000) if a.quick else (2000, 100000)
    ds = pdata.make_poi2vec_synthetic(n_user, n_item, 60, seed=20261016, local=0.8, box_km=1500.0)
    p = dict(latent_size=dim, seed=3, initial_alpha=0.01, softmax_axis="items", eval_context="test", batch_size_test=64)
    m = harness.poi2vec_model(ds, p)
    m.ctx.set_batch_cap(1)
    order = np.random.default_rng(0).permutation(ds.n_user)
    batches = [order[s:s + B] for s in range(0, ds.n_user, B)]
    batches = [b for b in batches if len(b) == B][:64]
    step = windows(lambda i: m.train_batch(batches[i % len(batches)], sync=False), len(batches), a.window_ms, a.repeats)
    m.ctx.timing(True)
    for b in batches:
        m.train_batch(b, sync=False)
    kt = {k: m.ctx.timing_get(k) for k in KERNELS}
    m.ctx.timing(False)
    rejected = m.ctx.take_bad_ids(m._stream().value)
    W = dict(wl=m._wl.clone(), xu=m._xu.clone(), pb=m._pb.clone())
    lds = [torch_launch_data(m, b) for b in batches[:16]]
    yard = windows(lambda i: torch_step(m, W, lds[i % len(lds)]), len(lds), a.window_ms, a.repeats)
    wl_bytes = 2 * 2 * ds.n_item * dim * 4            # wl read and written, twice (logsumexp pass + update pass)
    kern_us = {k: round(1e3 * v[0] / max(v[1], 1), 1) for k, v in kt.items() if v[1]}
    # top-20 of every user, 64 users per call
    m.update_trained_params()
    ses = harness.compute_start_end(ds.n_user, 64)
    top = windows(lambda i: m.compute_sub_topk(ses[i % len(ses)], 20), len(ses), a.window_ms, a.repeats)
    m.ctx.timing(True)
    for se in ses:
        m.compute_sub_topk(se, 20)
    st = {k: m.ctx.timing_get(k) for k in SC_KERNELS}
    m.ctx.timing(False)
    return {"dim": dim, "users": ds.n_user, "n_item": ds.n_item, "n_node": ds.n_node, "depth": ds.depth, "launch_users": B,
            "positions_per_launch": float(np.mean([m._lens[b].sum() for b in batches])),
            "step_wall_per_launch": step, "step_kernels_sum_us": round(sum(kern_us.values()), 1), "kernels_us_per_launch": kern_us,
            "wl_bytes_twice": wl_bytes, "wl_GBps_at_wall_median": wl_bytes / (step["median_ms"] * 1e-3) / 1e9,
            "torch_batched_per_launch": yard, "wall_median_ratio_torch_over_hip": yard["median_ms"] / step["median_ms"],
            "top20_per_64_users": top, "top20_all_users_ms_at_median": top["median_ms"] * len(ses),
            "score_kernels_us_per_64_rows": {k: round(1e3 * v[0] / max(v[1], 1), 1) for k, v in st.items() if v[1]},
            "score_node_product_flop_per_64_rows": 2 * 64 * ds.n_node * dim, "rejected": rejected,
            "finite": bool(torch.isfinite(m._wl).all() and torch.isfinite(m._xu).all() and torch.isfinite(m._pb).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    out = [run(d, B, a) for d in (20, 64) for B in (1, 64)]
    print(json.dumps({"bench": "poi2vec_step", "results": out}))


if __name__ == "__main__":
    main()
