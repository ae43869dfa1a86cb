"""float64 oracle of the fold-in rule (include/poi_hip.h, poi_foldin_bpr; public/BPR.py:216-230 and :287-306 with the item side frozen),
in plain loops on float32-rounded inputs.

    w = w0[r] (zeros without w0);  for e in range(epochs), for t in history order:
        d = Y[p_t] - Y[q_{e,t}],  x = w . d,  loss[r][e] += -log sigmoid(x),  w = w - alpha (-sigmoid(-x) d + lambda w)

q_{e,t} = q[e * q_epoch_stride + off[r] + t].  A user with descending offsets or an id outside [0, n_item] is a NaN row with NaN losses."""
import numpy as np


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x)) if x >= 0 else np.exp(x) / (1.0 + np.exp(x))


def neg_log_sigmoid(x):
    return max(-x, 0.0) + np.log1p(np.exp(-abs(x)))


def step(w, yp, yq, alpha, lam):
    """One check-in: (new w, -log sigmoid(x) at the old w)."""
    d = yp - yq
    x = float(np.dot(w, d))
    return w - alpha * (-sigmoid(-x) * d + lam * w), neg_log_sigmoid(x)


def fold_in(items, off, p, q, q_epoch_stride, epochs, alpha, lam, w0=None):
    """items (n_item + 1, dim) -> (w (n, dim), loss (n, epochs)) in float64; alpha / lam at their float32 values."""
    Y = f32(items)
    alpha, lam = float(np.float32(alpha)), float(np.float32(lam))
    n, n_item = len(off) - 1, Y.shape[0] - 1
    W = np.zeros((n, Y.shape[1])) if w0 is None else f32(w0).copy()
    loss = np.zeros((n, epochs))
    for r in range(n):
        a, b = int(off[r]), int(off[r + 1])
        ids = list(p[a:b]) + [q[e * q_epoch_stride + t] for e in range(epochs) for t in range(a, b)] if b >= a else []
        if b < a or a < 0 or any(i < 0 or i > n_item for i in ids):
            W[r] = np.nan; loss[r] = np.nan
            continue
        w = W[r]
        for e in range(epochs):
            for t in range(a, b):
                w, l = step(w, Y[p[t]], Y[q[e * q_epoch_stride + t]], alpha, lam)
                loss[r, e] += l
        W[r] = w
    return W, loss


# ---- seeded inputs shared by tests/test_foldin_cpu.py and tests/test_gpu_foldin.py ---------------------------------------------------
def toy(seed, dim, lens, epochs, n_item=50, hot=8):
    """Histories over few distinct POIs (rows repeat), per-epoch negatives, one planted p == q position per non-empty history, a
    float32-rounded item table with its padding row and a start row per user."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
    total = int(off[-1])
    p = rng.integers(0, hot, total)
    q = rng.integers(hot // 2, n_item + 1, max(epochs, 1) * total)
    for r, L in enumerate(lens):
        if L:
            q[off[r] + L // 2] = p[off[r] + L // 2]
    items = f32(rng.uniform(-0.5, 0.5, (n_item + 1, dim)))
    w0 = f32(rng.uniform(-0.5, 0.5, (len(lens), dim)))
    return dict(off=off, p=p, q=q, total=total, items=items, w0=w0, n_item=n_item, dim=dim, lens=list(lens))


LEARN = dict(n=40, n_item=200, dim=32, length=8, alpha=0.05, lam=0.001, epochs=5)


def learn_problem():
    """The convergence inputs: 40 users with 8 distinct POIs each, one fixed draw of negatives outside the history, a small start row."""
    c = LEARN
    rng = np.random.default_rng(2024)
    hist = np.stack([rng.choice(c["n_item"], c["length"], replace=False) for _ in range(c["n"])])
    neg = np.zeros_like(hist)
    for r in range(c["n"]):
        neg[r] = rng.choice(np.setdiff1d(np.arange(c["n_item"]), hist[r]), c["length"])
    off = np.arange(c["n"] + 1, dtype=np.int64) * c["length"]
    items = f32(rng.uniform(-0.5, 0.5, (c["n_item"] + 1, c["dim"])))
    w0 = f32(rng.uniform(-0.05, 0.05, (c["n"], c["dim"])))
    return dict(hist=hist, off=off, p=hist.reshape(-1), q=neg.reshape(-1), items=items, w0=w0)
