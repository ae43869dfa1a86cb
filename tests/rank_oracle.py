"""float64 oracle of the exact target rank (include/poi_hip.h, poi_score_rank / poi_rank_scores).

    C(r)       = [0, n_item) minus the exclusion list of row r
    rank[r][i] = |{ j in C(r), j != t : s(r, j) > s(r, t) or (s(r, j) == s(r, t) and j < t) }|,   t = tgt[r][i]

-1 for a masked position, an excluded target and a target outside [0, n_item).  Besides the rank the oracle reports, per (row, target),
`a` = the number of other ranked POIs whose float64 score lies within 1e-6 max|score of the row| of the target's (the gap rule of
tests/test_gpu_fullsize.py, qualifying()): a float32 kernel must place every POI outside that band on the right side, so its rank lies
in [greater_clear, greater_clear + a], greater_clear = the POIs above the band - and equals `rank` exactly where a == 0."""
import numpy as np

GAP = 1e-6


def exclusion_mask(n, n_item, ex_off=None, ex=None):
    """(n, n_item) bool: True where POI j is ranked for row r."""
    m = np.ones((n, n_item), bool)
    if ex_off is not None:
        for r in range(n):
            m[r, np.asarray(ex[ex_off[r]:ex_off[r + 1]], np.int64)] = False
    return m


def ranks(scores, tgt, tmask, ex_off=None, ex=None):
    """scores (n, n_item) float64 -> dict(rank, count, score, a, greater_clear), the per-target arrays (n, len_t)."""
    sc = np.asarray(scores, np.float64)
    tgt = np.asarray(tgt, np.int64); tmask = np.asarray(tmask)
    n, N = sc.shape
    keep = exclusion_mask(n, N, ex_off, ex)
    rank = np.full(tgt.shape, -1, np.int64); a = np.zeros(tgt.shape, np.int64); clear = np.zeros(tgt.shape, np.int64)
    val = np.full(tgt.shape, -np.inf)
    ids = np.arange(N)
    for r in range(n):
        band = GAP * np.abs(sc[r]).max()
        for i in range(tgt.shape[1]):
            t = tgt[r, i]
            if not tmask[r, i] or t < 0 or t >= N or not keep[r, t]:
                continue
            s = sc[r, t]
            others = keep[r] & (ids != t)
            rank[r, i] = int((others & ((sc[r] > s) | ((sc[r] == s) & (ids < t)))).sum())
            near = others & (np.abs(sc[r] - s) <= band)
            a[r, i] = int(near.sum())
            clear[r, i] = int((others & ~near & (sc[r] > s)).sum())
            val[r, i] = s
    return dict(rank=rank, count=keep.sum(axis=1), score=val, a=a, greater_clear=clear)


def summary(rank, count):
    """mrr, mean rank and auc_full = mean of 1 - rank / (count - 1) over the ranked positions (float64)."""
    rank = np.asarray(rank, np.int64)
    ok = rank >= 0
    r = rank[ok].astype(np.float64)
    c = np.broadcast_to(np.asarray(count)[:, None], rank.shape)[ok].astype(np.float64)
    return dict(mrr=float((1.0 / (r + 1.0)).mean()), mean_rank=float(r.mean()), auc_full=float((1.0 - r / (c - 1.0)).mean()))


def rank_list(rank, tgt, k):
    """The (n, k) top-k list the ranks imply: target t at position rank, -1 elsewhere (input of evaluate.rank_metrics)."""
    rank = np.asarray(rank); tgt = np.asarray(tgt)
    out = np.full((rank.shape[0], k), -1, np.int64)
    for r in range(rank.shape[0]):
        for i in range(rank.shape[1]):
            if 0 <= rank[r, i] < k:
                out[r, rank[r, i]] = tgt[r, i]
    return out
