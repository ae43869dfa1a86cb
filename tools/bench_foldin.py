#!/usr/bin/env python
"""Fold-in of new users (poi_foldin_bpr, models.MfBasic.fold_in) at the Gowalla shape: 100 k POIs, dim 128, histories from the synthetic
length distribution (data.make_synthetic: lognormal, 4 .. 20 check-ins), calls of 1 / 64 / 4096 / 50 000 users at 1 and 10 epochs with
one fixed draw of negatives per epoch resident on the device.
Timed: the entry itself on device tensors (no upload, no draw, no host check), chained calls with ONE synchronisation at the end of a
window.  Per cell: microseconds per call as the median of --repeats windows of at least --window-ms each (min and max alongside) after a
warm-up window, and from the median microseconds per user and nanoseconds per step (a step = one check-in of one epoch).
Beside it the same rule in batched torch ops in float64 (a loop over epochs and positions t, gathers over the users that still have a
position t): the yardstick a user without the kernel would write.  Prints one JSON line.
    python tools/bench_foldin.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness
from poi_amd.models import _ptr


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


def torch_fold_in(items, off, p, q, epochs, alpha, lam):
    """The rule in batched float64 torch ops: users sorted by descending length, position t handled for the users that have one."""
    lens = (off[1:] - off[:-1]).long()
    order = torch.argsort(lens, descending=True)
    ls, start = lens[order], off[:-1].long()[order]
    w = torch.zeros((lens.numel(), items.shape[1]), dtype=torch.float64, device=items.device)
    alive = [int((ls > t).sum()) for t in range(int(ls.max()) if ls.numel() else 0)]
    total = p.numel()
    for e in range(epochs):
        for t, m in enumerate(alive):
            at = start[:m] + t
            d = items[p[at].long()].double() - items[q[e * total + at].long()].double()
            x = (w[:m] * d).sum(1, keepdim=True)
            w[:m] -= alpha * (-torch.sigmoid(-x) * d + lam * w[:m])
    out = torch.empty_like(w)
    out[order] = w
    return out.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 50 ms")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 50.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    p_ = harness.default_params()
    p_.update(latent_size=D, gru=0)
    m = harness.build_model(ds, p_, seed=5)
    m.update_trained_items()
    alpha, lam = 0.05, 0.001
    off_h = np.asarray(ds.off, np.int64)
    out = dict(shape=dict(users=U, pois=N, dim=D, mean_len=round(float(np.diff(off_h).mean()), 2)), cells=[])
    i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(m.device)
    for n in (1, 64, 4096, U):
        if n > U:
            continue
        total = int(off_h[n])
        off, p = i32(off_h[:n + 1]), i32(np.asarray(ds.tra_p)[:total])
        for epochs in (1, 10):
            q = torch.randint(0, N, (epochs * total,), dtype=torch.int32, device=m.device)
            w = torch.empty((n, D), dtype=torch.float32, device=m.device)
            call = lambda: m.ctx.check(m.lib.poi_foldin_bpr(m.ctx.handle, _ptr(m.trained_items.t), N, D, _ptr(off), _ptr(p), _ptr(q), total, n, epochs,
                                                             alpha, lam, None, _ptr(w), None, m._stream()))
            hip = windows(call, a.window_ms, a.repeats)
            ref = torch_fold_in(m.trained_items.t, off, p, q, epochs, alpha, lam)
            err = float((w - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
            tch = windows(lambda: torch_fold_in(m.trained_items.t, off, p, q, epochs, alpha, lam), a.window_ms, max(1, a.repeats // 2))
            steps = total * epochs
            out["cells"].append(dict(users=n, epochs=epochs, steps=steps, foldin=hip, us_per_user=round(hip["us"] / n, 3),
                                     ns_per_step=round(hip["us"] * 1e3 / steps, 2), torch=tch, ratio=round(tch["us"] / hip["us"], 2),
                                     max_rel_diff_vs_torch=err))
    assert m.ctx.take_bad_ids() == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
