#!/usr/bin/env python
"""GeoIE step (poi_geoie_step, public/GeoIE.py:129-188) at D = 20 and 64 on two shapes: the synthetic Gowalla shape (make_synthetic,
local = 0.8; launches of 1024 users) and a long-sequence shape (2000 users, lognormal lengths up to 1264; launches of 64 users).  Prints one
JSON line: pairs/s of the step, the per-kernel times (timing names of include/poi_hip.h), a torch-ops yardstick of the same rule (padded
per-launch masked tensors, autograd backward) and the row-0 top-20 time for all users.  The scoring block ("score") times the top-20 under
the TRAINED rule (poi_geoie_score_topk_geo) for 1 / 64 / 4096 histories and for all users, beside the reference-rule
top-20 of the same users and the same rule in batched float64 torch ops (1 and 64 histories).
    python tools/bench_geoie.py [--launches N] [--quick] [--score-only]"""
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


def torch_geo_topk(m, users, k=20):
    """The trained rule in batched float64 torch ops on padded (B, Lmax, n_item) tensors + torch.topk (the yardstick)."""
    co, cp, cm = (t.long() for t in m._geo_train_csr())
    u = torch.as_tensor(np.asarray(users, np.int64), device=m.device)
    beg, ln = co[u], co[u + 1] - co[u]
    Lm = int(ln.max())
    pos = torch.arange(Lm, device=m.device)[None, :]
    ok = pos < ln[:, None]
    at = (beg[:, None] + pos).clamp(max=cp.numel() - 1)
    ids = torch.where(ok, cp[at], torch.zeros_like(at))
    mult = torch.where(ok, cm[at], torch.zeros_like(at)).double()
    g, h, z, t = (m._trained[k_] for k_ in ("g", "h", "z", "t"))
    n = m.n_item
    xy, cph, deg = m.coords, m._cphi, 0.017453292519943295
    a = (xy[ids, 0][:, :, None] - xy[None, None, :n, 0]) * deg
    b = (xy[ids, 1][:, :, None] - xy[None, None, :n, 1]) * deg
    c = (1.0 - torch.cos(a)) / 2 + cph[ids][:, :, None] * cph[None, None, :n] * (1.0 - torch.cos(b)) / 2
    d = (12742 * torch.asin(torch.sqrt(c))).float().double().clamp(min=m.d_min)
    f = m.ab[0] * torch.exp(m.ab[1] * torch.log(d))
    x = torch.matmul(g[ids], h[:n].t()).double()
    sc = (t[u] @ z[:n].t()).double() + (mult[:, :, None] * x * f).sum(1) / mult.sum(1).clamp(min=1)[:, None]
    return torch.topk(sc.float(), k, dim=1)


def score_block(m, ds):
    """Top-20 under both rules for 1 / 64 / 4096 / all users: ms per call, and pairs/s (distinct history POIs x candidates) of the geo rule."""
    def timed(fn, reps):
        fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    co = m._geo_train_csr()[0].cpu().numpy().astype(np.int64)
    distinct = np.diff(co)
    out = {}
    for n in (1, 64, 4096, ds.n_user):
        n = min(n, ds.n_user)
        se = np.arange(n, dtype=np.int32)
        reps = 20 if n <= 64 else 3 if n <= 4096 else 1
        geo = timed(lambda: m.compute_sub_topk(se, 20, rule="geo"), reps)
        ref = timed(lambda: m.compute_sub_topk(se, 20, rule="reference"), reps)
        pairs = float(distinct[:n].sum()) * ds.n_item
        rec = {"geo_ms": 1e3 * geo, "reference_ms": 1e3 * ref, "pairs": pairs, "geo_pairs_per_s": pairs / geo,
               "spans_per_row": m.ctx.last_plan("geoie_score_splits")}
        if n <= 64:
            tt = timed(lambda: torch_geo_topk(m, se), 3)
            rec.update(torch_ms=1e3 * tt, speedup_vs_torch=tt / geo)
        out["all" if n == ds.n_user and n > 4096 else str(n)] = rec
    idx, sc = m.compute_sub_topk(np.arange(min(64, ds.n_user), dtype=np.int32), 20, return_scores=True, rule="geo")
    ti = torch_geo_topk(m, np.arange(min(64, ds.n_user)))
    out["top20_overlap_with_torch"] = float((idx.long()[:, :, None] == ti.indices[:, None, :]).any(2).float().mean())
    return out


def run(shape, dim, launches, quick, score_only=False):
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
    if score_only:
        m.train_batch(np.arange(min(1024, ds.n_user)), sync=False)
        m.update_trained()
        return {"shape": shape, "dim": dim, "users": ds.n_user, "n_item": ds.n_item, "score": score_block(m, ds)}
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
    score = score_block(m, ds)
    return {"shape": shape, "dim": dim, "users": ds.n_user, "launch_users": B, "score": score, "launches": len(batches), "pairs": pairs,
            "ms_per_launch": 1e3 * dt / len(batches), "pairs_per_s": pairs / dt,
            "kernels_us_per_launch": {k: round(1e3 * v[0] / max(v[1], 1), 1) for k, v in kt.items() if v[1]},
            "torch_ms_per_launch": 1e3 * dtt, "torch_pairs_per_s": tpairs / dtt, "speedup_vs_torch": (tpairs / dtt and (pairs / dt) / (tpairs / dtt)),
            "top20_all_users_ms": 1e3 * dtop, "rejected": rejected, "finite": bool(torch.isfinite(m.g.t).all() and torch.isfinite(m.h.t).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--score-only", action="store_true", help="the scoring block only (skips the step and its torch yardstick)")
    a = ap.parse_args()
    out = [run(s, d, a.launches, a.quick, a.score_only) for s in ("gowalla", "long") for d in (20, 64)]
    print(json.dumps({"bench": "geoie_step", "results": out}))


if __name__ == "__main__":
    main()
