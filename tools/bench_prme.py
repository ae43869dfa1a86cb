#!/usr/bin/env python
"""PRME (prog_prme.py, public/PRME.py) at the Gowalla shape: the snapshot step in launches of --batch transitions at D = 20 and 64 against the
same rule written in torch ops, the per-user row-0 top-K evaluation of all users (poi_prme_score_topk), the full per-position scoring in the
reference's layout (batch_size_test users per call, poi_prme_score_all), a float64 torch yardstick for the scoring, and the split of the
per-pair scoring cost between the float64 weight and the float32 distances (time of one scoring call at D = 4 .. 128, fitted t = t0 + c D:
t0 is the D-independent part - the weight, plus the 4-byte store).
    python tools/bench_prme.py [--batch N] [--shape gowalla] [--epochs 3] [--score-batches 100]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import poi_amd
from poi_amd import data as pdata
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536); ap.add_argument("--shape", default="gowalla"); ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--cap", type=float, default=64.0); ap.add_argument("--dims", default="20,64"); ap.add_argument("--score-batches", type=int, default=100)
ap.add_argument("--batch-size-test", type=int, default=20); ap.add_argument("--box-km", type=float, default=300.0)
a = ap.parse_args()
n_item, n_user, max_len, _ = pdata.SHAPES[a.shape]
t0 = time.perf_counter()
ds = pdata.make_prme_synthetic(n_user, n_item, max_len, seed=20261016, local=0.8, box_km=a.box_km)
sync = torch.cuda.synchronize
out = {"shape": a.shape, "n_item": ds.n_item, "n_user": ds.n_user, "launch_transitions": a.batch, "cap": a.cap, "data_s": time.perf_counter() - t0}


def timed(f, reps):
    f(); sync(); t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    sync()
    return (time.perf_counter() - t0) / reps, r


def torch_step(T, u, p, q, v, d, gap, alpha, lam, cap, thd=360, cw=0.2):
    """The snapshot rule of poi_prme_step in torch ops (gathers, per-transition updates with the last-wins collapse as masks, index_add_ of
    the sums and touch counts - float atomics -, then row += min(k, cap) / k * sum)."""
    du, dp, ds_ = T["du"], T["dp"], T["ds"]
    U, Pp, Pq, Pv = du.index_select(0, u), dp.index_select(0, p), dp.index_select(0, q), dp.index_select(0, v)
    Sp, Sq, Sv = ds_.index_select(0, p), ds_.index_select(0, q), ds_.index_select(0, v)
    w = torch.sqrt(torch.sqrt(1.0 + d)).float()
    far = gap > thd
    A = torch.where(far, torch.ones_like(w), w * cw)[:, None]
    B = torch.where(far, torch.zeros_like(w), w * (1 - cw))[:, None]
    x = (A * ((U - Pq) ** 2) + B * ((Sq - Sv) ** 2) - A * ((U - Pp) ** 2) - B * ((Sp - Sv) ** 2)).sum(1)
    g = torch.sigmoid(-x)[:, None]
    loss = torch.nn.functional.logsigmoid(x)
    keep_p, keep_q = (p != v).float()[:, None], (q != v).float()[:, None]
    one = torch.ones_like(x)
    for tab, rows, dl, keep in ((du, (u,), (alpha * (2 * A * g * (Pp - Pq) - lam * U),), (None,)),
                                (dp, (p, q, v), (alpha * (2 * A * g * (U - Pp) - lam * Pp), alpha * (-2 * A * g * (U - Pq) - lam * Pq), -alpha * lam * Pv),
                                 (keep_p, keep_q, None)),
                                (ds_, (p, q, v), (alpha * (-2 * B * g * (Sp - Sv) - lam * Sp), alpha * (2 * B * g * (Sq - Sv) - lam * Sq),
                                                  alpha * (2 * B * g * (Sp - Sq) - lam * Sv)), (keep_p, keep_q, None))):
        acc = torch.zeros_like(tab); k = torch.zeros(tab.shape[0], device=tab.device)
        for r, val, kp in zip(rows, dl, keep):
            acc.index_add_(0, r, val if kp is None else val * kp); k.index_add_(0, r, one if kp is None else kp[:, 0])
        tab += (torch.clamp(k, max=cap) / k.clamp(min=1))[:, None] * acc
    return loss


def model(D):
    return poi_amd.models.OboPrme(train=ds, test=None, alpha_lambda=[0.01, 0.001], threshold=360, component_weight=0.2, cordi=ds.coords,
                                  n_user=ds.n_user, n_item=ds.n_item, n_size=D, seed=7)


for D in [int(x) for x in a.dims.split(",")]:
    m = model(D)
    m.ctx.set_batch_cap(a.cap)
    u, p, q, v, d, g = m.epoch_transitions(1, np.random.default_rng(1).permutation(ds.n_user))
    n = u.numel()
    B = a.batch or n

    def epoch():
        for b0 in range(0, n, B):
            s = slice(b0, b0 + B)
            m.train_batch(u[s], p[s], q[s], v[s], d[s], g[s], sync=False)
    dt, _ = timed(epoch, a.epochs)
    m.ctx.timing(True); epoch(); sync()
    launches = (n + B - 1) // B
    kt = {k: round(1e3 * m.ctx.timing_get(k)[0] / launches, 1) for k in ("prme_fwd", "prme_sort", "prme_rows", "prme_commit")}
    m.ctx.timing(False)
    assert m.ctx.take_bad_ids() == 0
    T = {k: getattr(m, k).t.clone() for k in ("du", "dp", "ds")}

    def tepoch():
        for b0 in range(0, n, B):
            s = slice(b0, b0 + B)
            torch_step(T, u[s].long(), p[s].long(), q[s].long(), v[s].long(), d[s], g[s], 0.01, 0.001, a.cap)
    dtt, _ = timed(tepoch, max(1, a.epochs // 2))
    out["step_D%d" % D] = {"transitions_per_epoch": n, "ms_per_epoch": 1e3 * dt, "transitions_per_s": n / dt, "kernel_us_per_launch": kt,
                           "torch_ops_ms_per_epoch": 1e3 * dtt, "torch_ops_transitions_per_s": n / dtt, "speedup_vs_torch_ops": dtt / dt,
                           "finite": bool(all(torch.isfinite(getattr(m, k).t).all() for k in ("du", "dp", "ds")))}
    del m

# ---- scoring at D = 20 (the reference's latent_size) -------------------------------------------------------------------------------
m = model(20)
m.update_trained_items()
N = ds.n_item
allu = np.arange(ds.n_user, dtype=np.int32)
dt, idx = timed(lambda: m.compute_sub_topk(allu, 20), 3)
out["eval_row0_topk20"] = {"users": ds.n_user, "ms": 1e3 * dt, "pairs_per_s": ds.n_user * N / dt}

ses = [np.arange(s, min(s + a.batch_size_test, ds.n_user), dtype=np.int32) for s in range(0, ds.n_user, a.batch_size_test)][:a.score_batches]
rows = 0


def full():
    global rows
    rows = 0
    for se in ses:
        rows += m.compute_sub_all_scores_device(se).shape[0]
dt, _ = timed(full, 1)
out["score_all_reference_layout"] = {"calls": len(ses), "users_per_call": a.batch_size_test, "rows": rows, "ms": 1e3 * dt,
                                     "pairs_per_s": rows * N / dt, "all_users_s_estimate": dt * ds.n_user / (len(ses) * a.batch_size_test)}

# one large call of row-0 rows at D = 4 .. 128: the weight's share of the per-pair cost
nr = 2048
uu = torch.as_tensor(allu[:nr]).cuda()
qq = m.tra_last_poi[:nr].contiguous()
ts = {}
for D in (4, 20, 64, 128):
    mm = m if D == 20 else model(D)
    mm.update_trained_items()
    ts[D], _ = timed(lambda: mm.score_rows_device(uu, qq), 5)
Ds = np.array(sorted(ts)); tt = np.array([ts[k] for k in Ds])
c1, c0 = np.polyfit(Ds, tt, 1)
out["score_cost_split"] = {"rows": nr, "ms_by_dim": {int(k): round(1e3 * ts[k], 3) for k in Ds}, "pairs_per_s_by_dim": {int(k): nr * N / ts[k] for k in Ds},
                           "fit_ms_fixed": 1e3 * c0, "fit_ms_per_dim": 1e3 * c1, "weight_share_D20": c0 / (c0 + 20 * c1), "weight_share_D64": c0 / (c0 + 64 * c1)}

# float64 torch yardstick of the same scores (200 rows)
r64 = 200
P64 = {k: m._trained[k].double() for k in ("du", "dp", "ds")}
xy = m.cordi


def torch64():
    ql = qq[:r64].long()
    U, S = P64["du"][uu[:r64].long()], P64["ds"][ql]
    Dp = torch.cdist(U, P64["dp"][:N]) ** 2
    Dsq = torch.cdist(S, P64["ds"][:N]) ** 2
    rad = lambda x: x * np.pi / 180.0
    r1, r2 = rad(xy[ql, 0])[:, None], rad(xy[:N, 0])[None, :]
    aa, bb = r1 - r2, rad(xy[ql, 1])[:, None] - rad(xy[:N, 1])[None, :]
    w = (1 + 2 * torch.asin(torch.sqrt(torch.sin(aa / 2) ** 2 + torch.cos(r1) * torch.cos(r2) * torch.sin(bb / 2) ** 2)) * 6378.137) ** 0.25
    return -w * (0.2 * Dp + 0.8 * Dsq)
dt64, ref = timed(torch64, 3)
got = m.score_rows_device(uu[:r64], qq[:r64]).double()
dtk, _ = timed(lambda: m.score_rows_device(uu[:r64], qq[:r64]), 5)
out["score_torch_f64_yardstick"] = {"rows": r64, "torch_f64_ms": 1e3 * dt64, "kernel_ms": 1e3 * dtk, "speedup": dt64 / dtk,
                                    "max_rel_err_vs_f64": float(((got - ref).abs() / ref.abs()).max().item())}
print(json.dumps(out))
