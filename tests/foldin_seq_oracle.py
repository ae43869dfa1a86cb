"""float64 oracle of fold-in for the successive-POI models (include/poi_hip.h, poi_foldin_terms_fpmc / poi_foldin_terms_prme /
poi_foldin_pair; public/FPMC_LR.py:113-140 and public/PRME.py:173-214 with the item side frozen), in plain loops on float32-rounded inputs.

A history p[off[r] .. off[r + 1]) of length L has the transitions t = 1 .. L - 1 with prev = p[t - 1], target p[t] and negative
q_{e,t} = q[e * q_epoch_stride + off[r] + t]; position 0 is no step.

    FPMC-LR:  c = ai[prev] . (ia[p_t] - ia[q]),  x = w . (iu[p_t] - iu[q]) + c,  w -= alpha (-sigmoid(-x) (iu[p_t] - iu[q]) + lambda w)
    PRME:     far = gap_t > thd,  wgt = (1 + d_t)^0.25,  a = far ? 1 : wgt cw,  b = far ? 0 : wgt (1 - cw)
              c = b (|ds[q] - ds[prev]|^2 - |ds[p_t] - ds[prev]|^2),  x = a (|w - dp[q]|^2 - |w - dp[p_t]|^2) + c
              w += alpha (sigmoid(-x) 2 a (dp[p_t] - dp[q]) - lambda w)
    loss[r][e] += -log sigmoid(x) in both

A negative of -1 skips its step (no update, no decay, no loss).  A user with descending offsets, any other id outside [0, n_item] or a
distance that is negative or not finite is a NaN row with NaN losses."""
import numpy as np

from tests.foldin_oracle import f32, neg_log_sigmoid, sigmoid
from tests.prme_oracle import cal_dis

DOT, METRIC = 0, 1


def step(form, w, yp, yq, a, c, alpha, lam):
    """One transition on the row: (new w, -log sigmoid(x) at the old w)."""
    d = yp - yq
    if form == DOT:
        x = float(np.dot(w, d)) + c
        g = sigmoid(-x)
    else:
        x = a * (float(((w - yq) ** 2).sum()) - float(((w - yp) ** 2).sum())) + c
        g = sigmoid(-x) * 2.0 * a
    return w - alpha * (-g * d + lam * w), neg_log_sigmoid(x)


def fpmc_terms(ia, ai, p, prev, q):
    """(c, sum of the absolute terms) of one FPMC-LR transition."""
    t = f32(ai)[prev] * (f32(ia)[p] - f32(ia)[q])
    return float(t.sum()), float(np.abs(t).sum())


def prme_terms(ds, p, prev, q, d, gap, thd, cw):
    """(a, c, sum of the absolute terms of c) of one PRME transition; cw at its float32 value."""
    cw = float(np.float32(cw))
    S = f32(ds)
    far = gap > thd
    wgt = (1.0 + d) ** 0.25
    a, b = (1.0, 0.0) if far else (wgt * cw, wgt * (1.0 - cw))
    tq, tp = (S[q] - S[prev]) ** 2, (S[p] - S[prev]) ** 2
    return a, b * float((tq - tp).sum()), b * float((tq + tp).sum())


def _bad_id(i, n_item):
    return i < 0 or i > n_item


def terms(model, T, off, p, q, q_epoch_stride, epochs, gap=None, dist=None, cordi=None, thd=360, cw=0.2):
    """The terms pass over a whole CSR -> dict(a (total), c (n_epoch x total), mass (like c): the sum of the absolute terms).
    model "fpmc": T holds ia / ai; "prme": T holds ds, with gap and dist or cordi.  Position 0 of a history is 0; entries with a
    rejected id or distance are NaN; a negative of -1 gives c = 0."""
    total = int(off[-1])
    n_item = len(T["ia" if model == "fpmc" else "ds"]) - 1
    ne = epochs if q_epoch_stride else 1
    a = np.zeros(total); c = np.zeros((ne, total)); mass = np.zeros((ne, total))
    for r in range(len(off) - 1):
        for t in range(int(off[r]) + 1, int(off[r + 1])):
            pt, pv = int(p[t]), int(p[t - 1])
            bad = _bad_id(pt, n_item) or _bad_id(pv, n_item)
            if model == "prme":
                d = float(dist[t]) if dist is not None else (np.nan if bad else float(cal_dis(cordi[pt, 0], cordi[pt, 1], cordi[pv, 0], cordi[pv, 1])))
                bad = bad or not np.isfinite(d) or d < 0
            for e in range(ne):
                qt = int(q[e * q_epoch_stride + t])
                if bad or (qt != -1 and _bad_id(qt, n_item)):
                    c[e, t] = np.nan
                    if model == "prme" and bad:
                        a[t] = np.nan
                    continue
                if model == "prme":
                    if qt == -1:
                        a[t] = prme_terms(T["ds"], pt, pv, pt, d, int(gap[t]), thd, cw)[0]
                    else:
                        a[t], c[e, t], mass[e, t] = prme_terms(T["ds"], pt, pv, qt, d, int(gap[t]), thd, cw)
                elif qt != -1:
                    c[e, t], mass[e, t] = fpmc_terms(T["ia"], T["ai"], pt, pv, qt)
    return dict(a=a, c=c, mass=mass)


def chain(form, items, off, p, q, q_epoch_stride, epochs, alpha, lam, a=None, c=None, c_epoch_stride=0, w0=None, first=1):
    """poi_foldin_pair: items (n_item + 1, dim) -> (w (n, dim), loss (n, epochs)) in float64; alpha / lam at their float32 values;
    a (total) or None = 1, c flat (epoch e at c[e * c_epoch_stride + pos]) or None = 0."""
    Y = f32(items)
    alpha, lam = float(np.float32(alpha)), float(np.float32(lam))
    n, n_item = len(off) - 1, Y.shape[0] - 1
    W = np.zeros((n, Y.shape[1])) if w0 is None else f32(w0).copy()
    loss = np.zeros((n, epochs))
    for r in range(n):
        lo, hi = int(off[r]), int(off[r + 1])
        if hi < lo or lo < 0:
            W[r] = np.nan; loss[r] = np.nan
            continue
        w, bad = W[r], first == 1 and hi > lo and _bad_id(int(p[lo]), n_item)
        for e in range(epochs):
            for t in range(lo + first, hi):
                pt, qt = int(p[t]), int(q[e * q_epoch_stride + t])
                at = 1.0 if a is None or form == DOT else float(a[t])
                ct = 0.0 if c is None else float(c[e * c_epoch_stride + t])
                if _bad_id(pt, n_item) or (qt != -1 and _bad_id(qt, n_item)) or not np.isfinite(at) or not np.isfinite(ct):
                    bad = True
                    continue
                if qt == -1:
                    continue
                w, l = step(form, w, Y[pt], Y[qt], at, ct, alpha, lam)
                loss[r, e] += l
        W[r] = w
        if bad:
            W[r] = np.nan; loss[r] = np.nan
    return W, loss


def fold_in_fpmc(T, off, p, q, q_epoch_stride, epochs, alpha, lam, w0=None):
    """OboFpmc_lr.fold_in: T holds iu / ia / ai."""
    tm = terms("fpmc", T, off, p, q, q_epoch_stride, epochs)
    return chain(DOT, T["iu"], off, p, q, q_epoch_stride, epochs, alpha, lam, None, tm["c"].reshape(-1), q_epoch_stride, w0)


def fold_in_prme(T, off, p, q, q_epoch_stride, epochs, alpha, lam, gap, dist=None, cordi=None, thd=360, cw=0.2, w0=None):
    """OboPrme.fold_in: T holds dp / ds."""
    tm = terms("prme", T, off, p, q, q_epoch_stride, epochs, gap, dist, cordi, thd, cw)
    return chain(METRIC, T["dp"], off, p, q, q_epoch_stride, epochs, alpha, lam, tm["a"], tm["c"].reshape(-1), q_epoch_stride, w0)


# ---- seeded inputs shared by tests/test_foldin_seq_cpu.py and tests/test_gpu_foldin_seq.py -----------------------------------------------
THD = 360


def toy(seed, dim, lens, epochs, n_item=50, hot=8):
    """Histories over few distinct POIs (rows repeat; p == q and p == prev occur), per-epoch negatives, three float32-rounded item
    tables with their padding rows, per-check-in gaps on both sides of THD and exactly at it, distances, coordinates with the pad row,
    per-position a / c for the raw chain tests and a start row per user."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
    total = int(off[-1])
    ne = max(epochs, 1)
    p = rng.integers(0, hot, total)
    q = rng.integers(hot // 2, n_item + 1, ne * total)
    for r, L in enumerate(lens):
        if L >= 3:
            p[off[r] + 2] = p[off[r] + 1]                      # p == prev
        if L >= 2:
            q[off[r] + L // 2] = p[off[r] + L // 2]            # p == q
    tab = lambda: f32(rng.uniform(-0.5, 0.5, (n_item + 1, dim)))
    gap = rng.choice([5, 120, THD - 1, THD, THD + 1, 2000], max(total, 1))[:total]
    dist = rng.uniform(0.0, 30.0, total)
    cordi = np.stack((30.0 + rng.uniform(0, 0.3, n_item + 1), 120.0 + rng.uniform(0, 0.3, n_item + 1)), axis=1)
    cordi[n_item] = 0.0
    return dict(off=off, p=p, q=q, total=total, y=tab(), s=tab(), v=tab(), gap=gap, dist=dist, cordi=cordi,
                a=rng.uniform(0.3, 2.0, total), c=rng.uniform(-1.0, 1.0, ne * total),
                w0=f32(rng.uniform(-0.5, 0.5, (len(lens), dim))), n_item=n_item, dim=dim, lens=list(lens))


LEARN = dict(n=40, n_item=200, dim=32, length=9, alpha=0.05, lam=0.001, epochs=5, cw=0.8)      # (cw: PRME's weight of the du term)


def learn_problem():
    """The convergence inputs: 40 users with 9 distinct POIs each (8 transitions), one fixed draw of negatives outside the history,
    a small start row, gaps on both sides of THD."""
    c = LEARN
    rng = np.random.default_rng(2025)
    hist = np.stack([rng.choice(c["n_item"], c["length"], replace=False) for _ in range(c["n"])])
    neg = np.zeros_like(hist)
    for r in range(c["n"]):
        neg[r] = rng.choice(np.setdiff1d(np.arange(c["n_item"]), hist[r]), c["length"])
    off = np.arange(c["n"] + 1, dtype=np.int64) * c["length"]
    tab = lambda: f32(rng.uniform(-0.5, 0.5, (c["n_item"] + 1, c["dim"])))
    total = c["n"] * c["length"]
    cordi = np.stack((30.0 + rng.uniform(0, 0.3, c["n_item"] + 1), 120.0 + rng.uniform(0, 0.3, c["n_item"] + 1)), axis=1)
    cordi[c["n_item"]] = 0.0
    return dict(hist=hist, off=off, p=hist.reshape(-1), q=neg.reshape(-1), y=tab(), s=tab(), v=tab(),
                gap=rng.choice([30, 200, THD + 40], total), dist=rng.uniform(0.0, 20.0, total), cordi=cordi,
                w0=f32(rng.uniform(-0.05, 0.05, (c["n"], c["dim"]))))
