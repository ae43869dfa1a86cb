#!/usr/bin/env python
"""Mini-batch Lstm / Rnn step (poi_cell_step, public/GRU.py:525-605 / :682-760) on the synthetic Gowalla shape (make_synthetic, its
length distribution) at D = 20, 64, 128 and batches of 64, 512, 4096 users, and predict for 16 384 users.  Next to every figure stands
the same rule written in batched torch ops on the same GPU (padded masked scan to the batch's longest length, autograd backward, dense
and index_add updates) in float32 and float64.  Every time is the median of `--reps` launches after `--warmup`, with the min .. max
spread; launches are timed with device events around the whole step.  Prints one JSON line.
    python tools/bench_cells.py [--reps N] [--warmup N] [--quick] [--cells lstm,rnn]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata
from poi_amd import models

KERNELS = ("cell_plan", "cell_rec", "cell_wgrad", "cell_sort", "cell_rows", "cell_commit")


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


def padded(m, users):
    off, lens = m._off_host.astype(np.int64), m._lens[users]
    L = int(lens.max())
    P = np.full((len(users), L), m.n_item, np.int64); Q = P.copy()
    ph, qh = m.p.cpu().numpy(), m.q.cpu().numpy()
    for k, u in enumerate(users):
        P[k, :lens[k]] = ph[off[u]:off[u] + lens[k]]; Q[k, :lens[k]] = qh[off[u]:off[u] + lens[k]]
    dev = m.device
    return torch.as_tensor(P, device=dev), torch.as_tensor(Q, device=dev), torch.as_tensor(lens, device=dev)


def torch_step(m, cell, pi, qi, lens, dtype, alpha, lam):
    """The reference graph in batched torch ops (the yardstick): returns nothing, updates clones."""
    lt, ui, wh, bi = (getattr(m, k).t.to(dtype).clone().requires_grad_() for k in ("lt", "ui", "wh", "bi"))
    n, L = pi.shape
    xp, xq = lt[pi], lt[qi]
    h = torch.zeros(n, m.dim, dtype=dtype, device=m.device); c = torch.zeros_like(h)
    mask = (torch.arange(L, device=m.device)[None, :] < lens[:, None]).to(dtype)
    loss = 0
    for t in range(L):
        x = xp[:, t]
        loss = loss + (torch.nn.functional.logsigmoid((h * (x - xq[:, t])).sum(1)) * mask[:, t]).sum()
        if cell == "lstm":
            g = torch.einsum("gjd,nd->gnj", ui, x) + torch.einsum("gjd,nd->gnj", wh, h) + bi[:, None, :]
            i, f, gg, o = torch.sigmoid(g[0]), torch.sigmoid(g[1]), torch.tanh(g[2]), torch.sigmoid(g[3])
            c = f * c + i * gg
            h = o * torch.tanh(c)
        else:
            h = torch.sigmoid(x @ ui.T + h @ wh.T + bi)
    pad = float(m.len_max - L) * 2 * n
    cost = -loss / n + 0.5 * lam * ((xp ** 2).sum() + (xq ** 2).sum() + pad * (lt[m.n_item] ** 2).sum() + (ui ** 2).sum() + (wh ** 2).sum() + (bi ** 2).sum())
    g_lt, g_ui, g_wh, g_bi = torch.autograd.grad(cost, [lt, ui, wh, bi])
    with torch.no_grad():
        for th, g in ((ui, g_ui), (wh, g_wh), (bi, g_bi), (lt, g_lt)):
            th -= alpha * g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true"); ap.add_argument("--cells", default="lstm,rnn")
    ap.add_argument("--dims", default="20,64,128"); ap.add_argument("--batches", default="64,512,4096")
    a = ap.parse_args()
    n_item, n_user, max_len, _ = pdata.SHAPES["gowalla"]
    if a.quick:
        n_item, n_user = 5000, 4096
    ds = pdata.make_synthetic(n_user, n_item, max_len, seed=1, local=0.8)
    tab = ds.shard()
    res = dict(shape=dict(n_item=n_item, n_user=n_user, max_len=max_len, mean_len=round(float(ds.lens.mean()), 2)), reps=a.reps, rows=[])
    rng = np.random.default_rng(0)
    for cell in a.cells.split(","):
        for dim in (int(d) for d in a.dims.split(",")):
            m = getattr(models, {"lstm": "Lstm", "rnn": "Rnn"}[cell])(train=tab, test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user,
                                                                     n_item=ds.n_item, n_in=dim, n_hidden=dim, seed=3)
            for batch in (int(b) for b in a.batches.split(",")):
                users = rng.permutation(ds.n_user)[:batch].astype(np.int32)
                ids = torch.as_tensor(users, device=m.device)
                steps = int(np.maximum(m._lens[users] - 1, 0).sum())
                row = dict(cell=cell, dim=dim, batch=batch, cell_steps=steps)
                row["hip"] = timed(lambda: m.train_batch(ids, sync=False), a.reps, a.warmup)
                assert m.ctx.take_bad_ids(m._stream().value) == 0
                row["hip_us_per_sequence_step"] = round(row["hip"]["median_us"] / max(steps, 1), 4)
                row["grid"] = m.ctx.last_plan("cell_grid")
                m.ctx.timing(True)
                m.train_batch(ids, sync=False)
                row["kernels_us"] = {k: round(m.ctx.timing_get(k)[0] * 1e3, 1) for k in KERNELS}
                m.ctx.timing(False)
                pi, qi, ln = padded(m, users)
                for name, dt in (("torch_f32", torch.float32), ("torch_f64", torch.float64)):
                    row[name] = timed(lambda: torch_step(m, cell, pi, qi, ln, dt, 0.01, 0.001), max(3, a.reps // 2), 1)
                    row["speedup_vs_" + name] = round(row[name]["median_us"] / row["hip"]["median_us"], 2)
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            npred = min(16384, ds.n_user)
            m.update_trained_items()
            pu = np.arange(npred, dtype=np.int32)
            res["rows"].append(dict(cell=cell, dim=dim, predict_users=npred, hip=timed(lambda: m.predict_device(pu), a.reps, a.warmup)))
            print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
            del m
    print(json.dumps(res))


if __name__ == "__main__":
    main()
