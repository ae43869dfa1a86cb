#!/usr/bin/env python
"""FPMC-LR (prog_fpmc_lr.py, public/FPMC_LR.py) at the Gowalla shape: neighbour-set build (poi_fpmc_neighbor_counts / _fill), the
neighbour-restricted sampler, and the snapshot step in launches of --batch transitions at D = 20 and 64, with per-kernel times, bytes moved per
transition, and the same snapshot rule written in torch ops (index_select / index_add_) at the same launch size as a yardstick.
    python tools/bench_fpmc.py [--batch N] [--shape gowalla] [--box-km 300] [--ud 20] [--epochs 5]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import poi_amd
from poi_amd import data as pdata
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536); ap.add_argument("--shape", default="gowalla"); ap.add_argument("--box-km", type=float, default=300.0)
ap.add_argument("--ud", type=float, default=20.0); ap.add_argument("--epochs", type=int, default=5); ap.add_argument("--cap", type=float, default=64.0)
ap.add_argument("--dims", default="20,64")
a = ap.parse_args()
n_item, n_user, max_len, _ = pdata.SHAPES[a.shape]
ds = pdata.make_synthetic(n_user, n_item, max_len, seed=20261016, local=0.8, box_km=a.box_km)
sync = torch.cuda.synchronize
out = {"shape": a.shape, "n_item": n_item, "n_user": n_user, "box_km": a.box_km, "UD_km": a.ud, "launch_transitions": a.batch, "cap": a.cap}


def timed(f, reps):
    f(); sync(); t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    sync()
    return (time.perf_counter() - t0) / reps, r


def torch_step(T, u, aa, i, j, alpha, lam, cap):
    """The snapshot rule of poi_fpmc_step in torch ops: gathers, per-transition updates, index_add_ of the sums and of the touch counts (float
    atomics), then row += min(k, cap) / k * sum."""
    ui, iu, ia, ai = T["ui"], T["iu"], T["ia"], T["ai"]
    U, A = ui.index_select(0, u), ai.index_select(0, aa)
    Ii, Ij, Ai, Aj = iu.index_select(0, i), iu.index_select(0, j), ia.index_select(0, i), ia.index_select(0, j)
    dI, dA = Ii - Ij, Ai - Aj
    x = (U * dI).sum(1) + (A * dA).sum(1)
    s = torch.sigmoid(-x)[:, None]
    loss = torch.nn.functional.logsigmoid(x)
    one = torch.ones_like(x)
    for tab, rows, d in ((ui, (u,), (alpha * (s * dI - lam * U),)), (ai, (aa,), (alpha * (s * dA - lam * A),)),
                         (iu, (i, j), (alpha * (s * U - lam * Ii), alpha * (-s * U - lam * Ij))),
                         (ia, (i, j), (alpha * (s * A - lam * Ai), alpha * (-s * A - lam * Aj)))):
        acc = torch.zeros_like(tab); k = torch.zeros(tab.shape[0], device=tab.device)
        for r, v in zip(rows, d):
            acc.index_add_(0, r, v); k.index_add_(0, r, one)
        tab += (torch.clamp(k, max=cap) / k.clamp(min=1))[:, None] * acc
    return loss


for D in [int(x) for x in a.dims.split(",")]:
    m = poi_amd.models.OboFpmc_lr(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001], n_user=n_user, n_item=n_item, n_size=D, seed=7,
                                  coords=ds.coords, ud_km=a.ud)
    m.ctx.set_batch_cap(a.cap)
    r = {}
    if "neighbours" not in out:
        dt, (off, nbr) = timed(lambda: m.build_neighbors(), 3)
        cnt = np.diff(off.cpu().numpy())
        m.ctx.timing(True); m.build_neighbors(); sync()
        out["neighbours"] = {"total_pairs": int(cnt.sum()), "mean_per_poi": float(cnt.mean()), "min_per_poi": int(cnt.min()), "ms_build": 1e3 * dt,
                             "kernels_ms": {k: round(m.ctx.timing_get(k)[0], 3) for k in ("fpmc_nbr_count", "fpmc_nbr_fill")},
                             "reference_haversine_calls": n_item * n_item}
        m.ctx.timing(False)
    u, aa, i, j = m.epoch_transitions(1)
    n = u.numel()
    if "sampler" not in out:
        dt, _ = timed(lambda: m.sample_negatives(i, 5), 20)
        out["sampler"] = {"draws": n, "ms": 1e3 * dt, "draws_per_s": n / dt}
    B = a.batch or n

    def epoch():
        for b0 in range(0, n, B):
            m.train_batch(u[b0:b0 + B], aa[b0:b0 + B], i[b0:b0 + B], j[b0:b0 + B], sync=False)
    dt, _ = timed(epoch, a.epochs)
    m.ctx.timing(True); epoch(); sync()
    launches = (n + B - 1) // B
    kt = {k: round(1e3 * m.ctx.timing_get(k)[0] / launches, 1) for k in ("fpmc_fwd", "fpmc_sort", "fpmc_rows", "fpmc_commit")}
    m.ctx.timing(False)
    assert m.ctx.take_bad_ids() == 0
    # bytes per transition: forward 6 rows read + 16 B ids + loss / s; rows pass: partner rows (8 rows per transition: 2 each for ui / ai
    # touches, 1 for each of the 4 POI touches) + every touched row read and its new row written to the slot; commit: slot read + table write;
    # sort: 6 keys x (4 passes x ~16 B).  Unique rows are at most 6 per transition - the figure below uses 6 (an upper bound).
    row = 4 * D
    by = 6 * row + 24 + 8 * row + 6 * row * 2 + 6 * row * 2 + 6 * 64
    T = {k: getattr(m, k).t.clone() for k in ("ui", "iu", "ia", "ai")}

    def tepoch():
        for b0 in range(0, n, B):
            torch_step(T, u[b0:b0 + B].long(), aa[b0:b0 + B].long(), i[b0:b0 + B].long(), j[b0:b0 + B].long(), 0.01, 0.001, a.cap)
    dtt, _ = timed(tepoch, max(1, a.epochs // 2))
    r.update({"transitions_per_epoch": n, "ms_per_epoch": 1e3 * dt, "transitions_per_s": n / dt, "kernel_us_per_launch": kt,
              "bytes_per_transition_upper": by, "GBps_upper": by * n / dt / 1e9,
              "torch_ops_ms_per_epoch": 1e3 * dtt, "torch_ops_transitions_per_s": n / dtt, "speedup_vs_torch_ops": dtt / dt,
              "finite": bool(all(torch.isfinite(getattr(m, k).t).all() for k in ("ui", "iu", "ia", "ai")))})
    out["D%d" % D] = r
    del m
print(json.dumps(out))
