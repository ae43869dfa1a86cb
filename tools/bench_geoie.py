#!/usr/bin/env python
"""GeoIE step (poi_geoie_step, public/GeoIE.py:129-188) at D = 20 and 64 on two shapes: the synthetic Gowalla shape (make_synthetic,
local = 0.8; launches of 1024 users) and a long-sequence shape (2000 users, lognormal lengths up to 1264; launches of 64 users).  Prints one
JSON line: pairs/s of the step, the per-kernel times (timing names of include/poi_hip.h), a torch-ops yardstick of the same rule (padded
per-launch masked tensors, autograd backward) and the row-0 top-20 time for all users.
    python tools/bench_geoie.py [--launches N] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata
from poi_amd.models import OboGeoIE

KERNELS = ("geoie_plan", "geoie_row", "geoie_col", "geoie_user", "geoie_sort", "geoie_rows", "geoie_commit", "geoie_ab")


def torch_step(m, users):
    """The same rule with torch ops on padded (B, R, R) tensors: forward, autograd backward (the yardstick)."""
    off = m._off_host.astype(np.int64)
    lens = np.maximum(m._lens[users] - 1, 0)
    R = int(lens.max())
    B = len(users)
    idx = np.zeros((B, R + 1), np.int64)
    qdx = np.zeros((B, R + 1), np.int64)
    ph, qh = m.p.cpu().numpy(), m.q.cpu().numpy()
    for k, u in enumerate(users):
        L = lens[k] + 1
        idx[k, :L] = ph[off[u]:off[u] + L]; qdx[k, :L] = qh[off[u]:off[u] + L]
    dev = m.device
    pi, qi = torch.as_tensor(idx, device=dev), torch.as_tensor(qdx, device=dev)
    valid = torch.arange(R, device=dev)[None, :] < torch.as_tensor(lens, device=dev)[:, None]
    M = torch.tril(torch.ones(R, R, device=dev, dtype=torch.bool))[None] & valid[:, :, None] & valid[:, None, :]
    g = m.g.t.clone().requires_grad_(); h = m.h.t.clone().requires_grad_()
    ab = m.ab.clone().requires_grad_()
    xy, cp = m.coords, m._cphi
    deg = 0.017453292519943295

    def dist(src, dst):
        a = (xy[src, 0][:, None, :] - xy[dst, 0][:, :, None]) * deg
        b = (xy[src, 1][:, None, :] - xy[dst, 1][:, :, None]) * deg
        c = (1.0 - torch.cos(a)) / 2 + cp[src][:, None, :] * cp[dst][:, :, None] * (1.0 - torch.cos(b)) / 2
        return (12742 * torch.asin(torch.sqrt(c))).float().double()

    gp, hp, hq = g[pi[:, :R]], h[pi[:, 1:]], h[qi[:, 1:]]
    X, Y = torch.bmm(hp, gp.transpose(1, 2)).double(), torch.bmm(hq, gp.transpose(1, 2)).double()
    dp, dq = dist(pi[:, :R], pi[:, 1:]), dist(pi[:, :R], qi[:, 1:])
    one = torch.ones_like(dp)
    fp = torch.where(M, ab[0] * torch.where(M, dp, one) ** ab[1], 0 * one)
    fq = torch.where(M, ab[0] * torch.where(M, dq, one) ** ab[1], 0 * one)
    nh = torch.arange(1, R + 1, device=dev, dtype=torch.float64)
    diff = (X * fp - Y * fq).sum(2) / nh
    loss = (torch.nn.functional.logsigmoid(diff) * valid).sum()
    (-loss).backward()
    return float(loss.detach())


def run(shape, dim, launches, quick):
    if shape == "gowalla":
        n_item, n_user, max_len, _ = pdata.SHAPES["gowalla"]
        if quick:
            n_user = 8192
        ds = pdata.make_synthetic(n_user, n_item, max_len, seed=20261016, local=0.8)
        B = 1024
    else:
        ds = pdata.make_synthetic(500 if quick else 2000, 20000, 1264, seed=20261017, local=0.8)
        B = 64
    m = OboGeoIE(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_in=dim, n_hidden=dim,
                 coords=ds.coords, seed=3, d_min=0.01)
    m.ctx.set_batch_cap(1)
    order = np.random.default_rng(0).permutation(ds.n_user)
    batches = [order[s:s + B] for s in range(0, ds.n_user, B)][:launches]
    rows = [np.maximum(m._lens[b] - 1, 0) for b in batches]
    pairs = sum(int((r * (r + 1) // 2).sum()) for r in rows)
    for b in batches[:2]:
        m.train_batch(b, sync=False)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in batches:
        m.train_batch(b, sync=False)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    m.ctx.timing(True)
    for b in batches:
        m.train_batch(b, sync=False)
    kt = {k: m.ctx.timing_get(k) for k in KERNELS}
    m.ctx.timing(False)
    rejected = m.ctx.take_bad_ids(m._stream().value)
    # torch-ops yardstick on the first launches
    tb = batches[:min(len(batches), 3)]
    torch_step(m, tb[0])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in tb:
        torch_step(m, b)
    torch.cuda.synchronize(); dtt = (time.perf_counter() - t0) / len(tb)
    tpairs = sum(int((r * (r + 1) // 2).sum()) for r in rows[:len(tb)]) / len(tb)
    # row-0 top-20 of every user
    m.update_trained()
    ses = [np.arange(s, min(s + 4096, ds.n_user), dtype=np.int32) for s in range(0, ds.n_user, 4096)]
    for se in ses[:1]:
        m.compute_sub_topk(se, 20)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    m._uvec = None
    for se in ses:
        m.compute_sub_topk(se, 20)
    torch.cuda.synchronize(); dtop = time.perf_counter() - t0
    return {"shape": shape, "dim": dim, "users": ds.n_user, "launch_users": B, "launches": len(batches), "pairs": pairs,
            "ms_per_launch": 1e3 * dt / len(batches), "pairs_per_s": pairs / dt,
            "kernels_us_per_launch": {k: round(1e3 * v[0] / max(v[1], 1), 1) for k, v in kt.items() if v[1]},
            "torch_ms_per_launch": 1e3 * dtt, "torch_pairs_per_s": tpairs / dtt, "speedup_vs_torch": (tpairs / dtt and (pairs / dt) / (tpairs / dtt)),
            "top20_all_users_ms": 1e3 * dtop, "rejected": rejected, "finite": bool(torch.isfinite(m.g.t).all() and torch.isfinite(m.h.t).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    out = [run(s, d, a.launches, a.quick) for s in ("gowalla", "long") for d in (20, 64)]
    print(json.dumps({"bench": "geoie_step", "results": out}))


if __name__ == "__main__":
    main()
