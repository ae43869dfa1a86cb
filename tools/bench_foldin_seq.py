#!/usr/bin/env python
"""Fold-in of new users for the successive-POI models (poi_foldin_terms_fpmc / poi_foldin_terms_prme / poi_foldin_pair) at the Gowalla
shape: 100 k POIs, D = 20 and 64, histories from the synthetic length distribution (data.make_synthetic: lognormal, 4 .. 20 check-ins),
calls of 1 / 64 / 4096 / 50 000 users at 1 and 10 epochs with one fixed draw of negatives per epoch resident on the device; random
float32 tables, random gaps (a third beyond the threshold) and distances.
Timed: the entries themselves on device tensors (no upload, no draw, no host check) - the terms pass and the chain SEPARATELY -, chained
calls with ONE synchronisation at the end of a window.  Per cell: microseconds per call as the median of --repeats windows of at least
--window-ms each (min and max alongside) after a warm-up window, and from the medians microseconds per user and nanoseconds per step
(a step = one transition of one epoch).  Beside them the same rule - terms and chain - in batched torch ops in float64 (a loop over
epochs and positions t, gathers over the users that still have a position t): the yardstick a user without the kernels would write.
Prints one JSON line.
    python tools/bench_foldin_seq.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import _lib, data as pdata

THD, CW = 360, 0.2


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


def torch_fold_in(model, Y, S, V, off, p, q, gap, dist, epochs, alpha, lam):
    """Both rules in batched float64 torch ops: users sorted by descending length, transition t handled for the users that have one."""
    lens = (off[1:] - off[:-1]).long()
    order = torch.argsort(lens, descending=True)
    ls, start = lens[order], off[:-1].long()[order]
    w = torch.zeros((lens.numel(), Y.shape[1]), dtype=torch.float64, device=Y.device)
    alive = [int((ls > t).sum()) for t in range(1, int(ls.max()) if ls.numel() else 0)]
    total = p.numel()
    for e in range(epochs):
        for t, m in enumerate(alive, start=1):
            if not m:
                break
            at = start[:m] + t
            ip, iv, iq = p[at].long(), p[at - 1].long(), q[e * total + at].long()
            yp, yq = Y[ip].double(), Y[iq].double()
            d = yp - yq
            if model == "fpmc":
                c = (V[iv].double() * (S[ip].double() - S[iq].double())).sum(1, keepdim=True)
                x = (w[:m] * d).sum(1, keepdim=True) + c
                g = torch.sigmoid(-x)
            else:
                far = (gap[at] > THD)[:, None]
                wgt = (1.0 + dist[at])[:, None] ** 0.25
                a = torch.where(far, torch.ones_like(wgt), wgt * CW)
                b = torch.where(far, torch.zeros_like(wgt), wgt * (1.0 - CW))
                sv = S[iv].double()
                c = b * (((S[iq].double() - sv) ** 2).sum(1, keepdim=True) - ((S[ip].double() - sv) ** 2).sum(1, keepdim=True))
                x = a * (((w[:m] - yq) ** 2).sum(1, keepdim=True) - ((w[:m] - yp) ** 2).sum(1, keepdim=True)) + c
                g = torch.sigmoid(-x) * 2.0 * a
            w[:m] -= alpha * (-g * d + lam * w[:m])
    out = torch.empty_like(w)
    out[order] = w
    return out.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 30 ms")
    a = ap.parse_args()
    U, N = (4096, 10000) if a.quick else (50000, 100000)
    if a.quick:
        a.repeats, a.window_ms = 3, 30.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    ctx = _lib.context(0)
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    alpha, lam = 0.05, 0.001
    off_h = np.asarray(ds.off, np.int64)
    out = dict(shape=dict(users=U, pois=N, mean_len=round(float(np.diff(off_h).mean()), 2)), cells=[])
    i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for D in (20, 64):
        Y, S, V = (torch.rand((N + 1, D), generator=gen, device=dev, dtype=torch.float32) - 0.5 for _ in range(3))
        for n in (1, 64, 4096, U):
            if n > U:
                continue
            total = int(off_h[n])
            off, p = i32(off_h[:n + 1]), i32(np.asarray(ds.tra_p)[:total])
            gap = torch.where(torch.rand(total, generator=gen, device=dev) < 0.33, 2 * THD, THD // 3).int()
            dist = torch.rand(total, generator=gen, device=dev, dtype=torch.float64) * 20.0
            for epochs in (1, 10):
                q = torch.randint(0, N, (epochs * total,), dtype=torch.int32, device=dev)
                w = torch.empty((n, D), dtype=torch.float32, device=dev)
                c = torch.empty(epochs * total, dtype=torch.float64, device=dev)
                av = torch.empty(total, dtype=torch.float64, device=dev)
                steps = (total - n) * epochs
                for model in ("fpmc", "prme"):
                    if model == "fpmc":
                        P = _lib.FpmcParams(None, ptr(Y), ptr(S), ptr(V), 1, N, D)
                        terms = lambda: ctx.check(ctx.lib.poi_foldin_terms_fpmc(ctx.handle, ctypes.byref(P), ptr(off), ptr(p), ptr(q), total, n, total,
                                                                                epochs, ptr(c), st()))
                        form, a_arg = _lib.FOLDIN_DOT, None
                    else:
                        P = _lib.PrmeParams(None, ptr(Y), ptr(S), 1, N, D)
                        terms = lambda: ctx.check(ctx.lib.poi_foldin_terms_prme(ctx.handle, ctypes.byref(P), None, ptr(off), ptr(p), ptr(q), total,
                                                                                ptr(gap), ptr(dist), n, total, epochs, THD, CW, ptr(av), ptr(c), st()))
                        form, a_arg = _lib.FOLDIN_METRIC, av
                    chain = lambda: ctx.check(ctx.lib.poi_foldin_pair(ctx.handle, ptr(Y), N, D, form, 1, ptr(off), ptr(p), ptr(q), total, ptr(a_arg),
                                                                      ptr(c), total, n, epochs, alpha, lam, None, ptr(w), None, st()))
                    t_terms = windows(terms, a.window_ms, a.repeats)
                    t_chain = windows(chain, a.window_ms, a.repeats)
                    ref = torch_fold_in(model, Y, S, V, off, p, q, gap, dist, epochs, alpha, lam)
                    err = float((w - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
                    tch = windows(lambda: torch_fold_in(model, Y, S, V, off, p, q, gap, dist, epochs, alpha, lam), a.window_ms, max(1, a.repeats // 2))
                    both = t_terms["us"] + t_chain["us"]
                    out["cells"].append(dict(model=model, dim=D, users=n, epochs=epochs, steps=steps, terms=t_terms, chain=t_chain,
                                             us_per_user=round(both / n, 3), ns_per_step=round(both * 1e3 / max(steps, 1), 2), torch=tch,
                                             ratio=round(tch["us"] / both, 2), max_rel_diff_vs_torch=err))
    assert ctx.take_bad_ids() == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
