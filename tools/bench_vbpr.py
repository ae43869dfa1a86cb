#!/usr/bin/env python
"""VBPR step (poi_vbpr_step, public/BPR.py:268-319) on the synthetic Gowalla shape (make_synthetic) with a synthetic feature table
(data.synthetic_features, F = 1024) at D = 20, 64 and launches of 64, 4096, 65536 triples, and the update_trained_items product
[lt | fi ei^T].  Next to every figure stands the same batch rule written in batched torch ops on the same GPU (gathers, two matmuls over
the gathered difference matrix, index_add updates, float32).  Every time is the median of `--reps` launches after `--warmup`, with the
min .. max spread; launches are timed with device events around the whole step.  Reads nothing outside the repository.  Prints one JSON
line.
    python tools/bench_vbpr.py [--reps N] [--warmup N] [--quick]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata
from poi_amd import models

KERNELS = ("vbpr_fwd", "vbpr_wgrad", "vbpr_sort", "vbpr_rows", "vbpr_commit")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1), max_us=round(ts[-1], 1))


def torch_step(m, u, p, q, alpha, lam, lam_ev, cap):
    """the batch rule of include/poi_hip.h in batched torch ops (float32), in place on clones of the tables"""
    ux, lt, ue, ei, fi = m._t
    u, p, q = u.long(), p.long(), q.long()
    d = fi[p] - fi[q]
    v = d @ ei.T
    xd = lt[p] - lt[q]
    x = (ux[u] * xd).sum(1) + (ue[u] * v).sum(1)
    g = -torch.sigmoid(-x)
    n = u.numel()

    def rows(tab, idx, grad):
        G = torch.zeros_like(tab).index_add_(0, idx, grad)
        c = torch.zeros(tab.shape[0], device=tab.device).index_add_(0, idx, torch.ones(idx.numel(), device=tab.device))
        sc = (alpha * torch.clamp(c, max=cap) * (c > 0))[:, None]
        return tab - sc * (G / torch.clamp(c, min=1.0)[:, None] + lam * tab)
    uxu = ux[u]
    nux = rows(ux, u, g[:, None] * xd)
    nue = rows(ue, u, g[:, None] * v)
    nlt = rows(lt, torch.cat([p, q]), torch.cat([g[:, None] * uxu, -g[:, None] * uxu]))
    nei = ei - alpha * min(float(n), cap) * (((g[:, None] * ue[u]).T @ d) / n + lam_ev * ei)
    m._t = (nux, nlt, nue, nei, fi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    n_item, n_user, max_len, _ = pdata.SHAPES["tiny" if a.quick else "gowalla"]
    ds = pdata.make_synthetic(n_user, n_item, max_len, seed=1)
    F, cap = 1024, 8.0
    fea = pdata.synthetic_features(ds.n_item, F, 1, scale=1.0 / np.sqrt(F))
    out = dict(shape=dict(n_user=ds.n_user, n_item=ds.n_item, n_img=F, cap=cap), rows=[])
    for D in (20, 64):
        m = models.OboVBpr(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_in=D, n_hidden=D,
                           n_img=F, fea_img=fea, seed=3)
        m.ctx.set_batch_cap(cap)
        U, P, Q = m.epoch_triples()
        perm = torch.randperm(U.numel(), generator=torch.Generator().manual_seed(5)).to(m.device)
        U, P, Q = (t.index_select(0, perm).contiguous() for t in (U, P, Q))
        for n in (64, 4096, 65536):
            n = min(n, U.numel())
            u, p, q = U[:n].contiguous(), P[:n].contiguous(), Q[:n].contiguous()
            row = dict(D=D, n=n)
            row["hip"] = timed(lambda: m.train_batch(u, p, q, sync=False), a.reps, a.warmup)
            m.ctx.timing(True)
            m.train_batch(u, p, q, sync=False); torch.cuda.synchronize()
            row["kernels_us"] = {k: round(m.ctx.timing_get(k)[0] * 1e3, 1) for k in KERNELS}
            m.ctx.timing(False)
            m._t = tuple(t.t.clone() for t in (m.ux, m.lt, m.ue, m.ei, m.fi))
            row["torch_f32"] = timed(lambda: torch_step(m, u, p, q, 0.01, 0.001, 0.001, cap), a.reps, a.warmup)
            row["speedup_vs_torch_f32"] = round(row["torch_f32"]["median_us"] / row["hip"]["median_us"], 2)
            row["feature_bytes_per_pass"] = 2 * F * 4 * n
            out["rows"].append(row)
        it = dict(D=D, rows=ds.n_item + 1)
        it["hip"] = timed(m.update_trained_items, a.reps, a.warmup)
        it["torch_f32"] = timed(lambda: torch.cat([m.lt.t, m.fi.t @ m.ei.t.T], 1), a.reps, a.warmup)
        out.setdefault("items", []).append(it)
        m.ctx.set_batch_cap(1.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
