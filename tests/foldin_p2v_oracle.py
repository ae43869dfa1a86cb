"""Float64 numpy restatement of POI2Vec fold-in (include/poi_hip.h, poi_foldin_p2v), in plain loops on float32-rounded inputs.

In Poi2vec.seq_train (public/POI2Vec.py:140-163) paths_i depends on wl, pb and the contexts, never on xu.  With the item side frozen
the row of user u sees

    upq(w) = logsumexp_j (w . wl_j) - (1/L) sum_i w . wl_{t_i}          (+ mean_i -log paths_i, which does not depend on w)
    d cost / d w = sum_j plu_j wl_j - (1/L) sum_i wl_{t_i} + lambda w,   plu = softmax_j (w . wl_j),   j < n_item
    w <- w - alpha d cost / d w                                          one step per pass over the history

which is the xu[u] part of tests/poi2vec_oracle.step (tests/test_foldin_p2v_cpu.py holds the two together).  Also: the scores of a
folded row (poi2vec_oracle.scores_factorised with the softmax over the POIs) and the top-K under exclusion lists."""
import numpy as np

from tests import poi2vec_oracle as PO


def grad(wl, targets, w, lam):
    """(loss before the update, d cost / d w) for one row; wl (n_item, D) - no pad row."""
    wl = np.asarray(wl, np.float64)
    t = np.asarray(targets, np.int64)
    s = wl @ w
    m = s.max()
    e = np.exp(s - m)
    lse = m + np.log(e.sum())
    plu = e / e.sum()
    tbar = wl[t].sum(axis=0) / len(t)
    return lse - s[t].sum() / len(t), plu @ wl - tbar + lam * w


def fold_in(wl, histories, epochs, alpha, lam, w0=None):
    """-> (rows (n, D), losses (n, epochs)), float64.  alpha / lam at their float32 values, as the device takes them; an empty history
    or epochs = 0 returns w0 and losses 0; a history with an id outside [0, n_item) gives NaN."""
    wl = np.asarray(wl, np.float64)
    n, D = len(histories), wl.shape[1]
    alpha, lam = float(np.float32(alpha)), float(np.float32(lam))
    W = np.zeros((n, D)) if w0 is None else np.asarray(w0, np.float32).astype(np.float64).copy()
    losses = np.zeros((n, epochs))
    for r, h in enumerate(histories):
        h = np.asarray(h, np.int64)
        if h.size and (h.min() < 0 or h.max() >= len(wl)):
            W[r] = np.nan; losses[r] = np.nan
            continue
        if not h.size:
            continue
        w = W[r].copy()
        for e in range(epochs):
            losses[r, e], g = grad(wl, h, w, lam)
            w = w - alpha * g
        W[r] = w
    return W, losses


def context_rows(wl, histories, contexts):
    """The context sums cl (n, 1, D) of score_new: "last", "none" or one id list per history."""
    out = []
    for r, h in enumerate(histories):
        if isinstance(contexts, str):
            c = list(h[-1:]) if contexts == "last" else []
        else:
            c = contexts[r]
        out.append(PO.context_sum(wl, c))
    return np.stack(out)[:, None, :] if out else np.zeros((0, 1, wl.shape[1]))


def scores(P, T, W, histories, contexts="last"):
    """paths_j plu_j of the folded rows W (n, D), one row per history, plu the softmax over the POIs."""
    Q = dict(P, xu=np.asarray(W, np.float64))
    return PO.scores_factorised(Q, T, np.arange(len(W)), context_rows(P["wl"], histories, contexts), "items")


def history_exclusion(histories, n_item):
    """exclude="history": (ex_off, ex) - every history's distinct POIs, ascending."""
    off, ex = [0], []
    for h in histories:
        ex.extend(sorted({int(v) for v in h if 0 <= int(v) < n_item}))
        off.append(len(ex))
    return np.asarray(off, np.int32), np.asarray(ex, np.int32)


def topk_ex(score_rows, k, ex_off=None, ex=None):
    """Top-k per row of a score matrix with the excluded columns removed: (ids (n, k) with -1 past the candidates, counts (n))."""
    s = np.asarray(score_rows)
    n, N = s.shape
    idx = np.full((n, k), -1, np.int32)
    cnt = np.zeros(n, np.int32)
    for r in range(n):
        keep = np.ones(N, bool)
        if ex_off is not None:
            keep[np.asarray(ex[ex_off[r]:ex_off[r + 1]], np.int64)] = False
        cols = np.flatnonzero(keep)
        cnt[r] = len(cols)
        if len(cols):
            top = PO.topk_desc(s[r:r + 1, cols], min(k, len(cols)))[0]
            idx[r, :len(top)] = cols[top]
    return idx, cnt
