#!/usr/bin/env python
"""Fold-in of new users for POI2Vec (poi_foldin_p2v, models.OboPoi2vec.fold_in / recommend_new) at the shape of tools/bench_poi2vec.py:
the synthetic check-in set over a 1500 km box (make_poi2vec_synthetic, 2000 users drawing from 100 k POIs: the POIs that occur are the
table), histories = the users' train check-ins, repeated to fill calls of 1 / 64 / 4096 users, at 1 and 10 epochs, D = 20 / 64.
Timed: the entry itself on device tensors (no upload, no host check), chained calls with ONE synchronisation at the end of a window.  Per
cell: microseconds per call as the median of --repeats windows of at least --window-ms each (min and max alongside) after a warm-up
window; from the median the microseconds per user-epoch, the float64 matrix rate of the pass (4 n n_item D flop per epoch: logits + the
weighted row sums) and the bytes of wl the pass kernels read per epoch over the time.  The foldin_p2v_prep / _pass / _upd split comes from
the library's event timing in a separate run.
Beside it the same rule in batched float64 torch ops (softmax(W WL^T) @ WL per epoch): the yardstick a user without the kernel would
write.  Last section: recommend_new top-20 (fold-in, 10 epochs + poi_poi2vec_topk_ex) beside compute_sub_topk over as many trained users.
Prints one JSON line.
    python tools/bench_foldin_p2v.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import _lib, data as pdata, harness
from poi_amd.models import _ptr

KERNELS = ("foldin_p2v_prep", "foldin_p2v_pass", "foldin_p2v_upd")


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


def torch_fold_in(wl, off, p, epochs, alpha, lam):
    """The rule in batched float64 torch ops; tbar through one index_add over the check-ins."""
    n = off.numel() - 1
    lens = (off[1:] - off[:-1]).long()
    row = torch.repeat_interleave(torch.arange(n, device=wl.device), lens)
    WL = wl.double()
    tbar = torch.zeros((n, WL.shape[1]), dtype=torch.float64, device=wl.device).index_add_(0, row, WL[p.long()]) / lens.clamp(min=1)[:, None]
    w = torch.zeros_like(tbar)
    for _ in range(epochs):
        w = w - alpha * (torch.softmax(w @ WL.T, 1) @ WL - tbar + lam * w)
    return w.float()


def run(dim, a):
    n_user, n_pool = (600, 20000) if a.quick else (2000, 100000)
    ds = pdata.make_poi2vec_synthetic(n_user, n_pool, 60, seed=20261016, local=0.8, box_km=1500.0)
    p_ = dict(latent_size=dim, seed=3, initial_alpha=0.01, softmax_axis="items", eval_context="test", batch_size_test=64)
    m = harness.poi2vec_model(ds, p_)
    m.update_trained_params()
    N, wl = ds.n_item, m._trained["wl"]
    alpha, lam = 0.1, 0.001
    off_h = np.asarray(ds.off, np.int64)
    users = [u for u in range(ds.n_user) if off_h[u + 1] > off_h[u]]
    n_span = -(-N // _lib.P2V_FOLD_SPAN)
    i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(m.device)
    cells = []
    for n in ((1, 64, 512) if a.quick else (1, 64, 4096)):
        pick = [users[i % len(users)] for i in range(n)]
        hist = [np.asarray(ds.tra_t[off_h[u]:off_h[u + 1]]) for u in pick]
        oh = np.zeros(n + 1, np.int64)
        oh[1:] = np.cumsum([len(h) for h in hist])
        off, p = i32(oh), i32(np.concatenate(hist))
        for epochs in (1, 10):
            w = torch.empty((n, dim), dtype=torch.float32, device=m.device)
            call = lambda: m.ctx.check(m.lib.poi_foldin_p2v(m.ctx.handle, _ptr(wl), N, dim, _ptr(off), _ptr(p), n, epochs, alpha, lam, None, _ptr(w),
                                                             None, m._stream()))
            hip = windows(call, a.window_ms, a.repeats)
            m.ctx.timing(True)
            for _ in range(8):
                call()
            torch.cuda.synchronize()
            kt = {k: m.ctx.timing_get(k) for k in KERNELS}
            m.ctx.timing(False)
            kern_us = {k: round(1e3 * v[0] / 8, 2) for k, v in kt.items() if v[1]}      # per CALL: all epochs, all user chunks
            ref = torch_fold_in(wl[:N], off, p, epochs, alpha, lam)
            err = float((w - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
            tch = windows(lambda: torch_fold_in(wl[:N], off, p, epochs, alpha, lam), a.window_ms, max(1, a.repeats // 2))
            pass_us = kern_us.get("foldin_p2v_pass", 0.0) / epochs                          # per epoch
            groups = -(-n // 64)
            cells.append(dict(users=n, epochs=epochs, foldin=hip, us_per_user_epoch=round(hip["us"] / (n * epochs), 3), kernels_us_per_call=kern_us,
                              pass_f64_tflops=round(4.0 * n * N * dim / (pass_us * 1e-6) / 1e12, 3) if pass_us else None,
                              pass_wl_bytes_read=groups * N * dim * 4,
                              pass_wl_GBps=round(groups * N * dim * 4 / (pass_us * 1e-6) / 1e9, 1) if pass_us else None,
                              workgroups=groups * n_span, torch=tch, ratio=round(tch["us"] / hip["us"], 2), max_rel_diff_vs_torch=err))
    # recommend_new top-20 beside compute_sub_topk over as many trained users
    serve = []
    for n in (1, 64):
        hist = [np.asarray(ds.tra_t[off_h[u]:off_h[u + 1]]) for u in users[:n]]
        oh = np.zeros(n + 1, np.int64)
        oh[1:] = np.cumsum([len(h) for h in hist])
        csr = (i32(oh), i32(np.concatenate(hist)))
        new = windows(lambda: m.recommend_new(csr, 20, epochs=10, alpha=alpha, lam=lam, sync=False), a.window_ms, a.repeats)
        old = windows(lambda: m.compute_sub_topk(np.asarray(users[:n]), 20), a.window_ms, a.repeats)
        serve.append(dict(users=n, recommend_new_top20=new, compute_sub_topk_top20=old))
    assert m.ctx.take_bad_ids() == 0
    return dict(dim=dim, pois=N, spans=n_span, mean_len=round(float(np.diff(off_h).mean()), 2), cells=cells, serving=serve)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--quick", action="store_true", help="600 users / 20 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    print(json.dumps({"bench": "foldin_p2v", "results": [run(d, a) for d in (20, 64)]}))


if __name__ == "__main__":
    main()
