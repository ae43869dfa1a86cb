"""Numpy oracle of the re-ranking entries (include/poi_hip.h, poi_score_lists / poi_rerank_lists / poi_rerank).  Exact, no tolerance: it
reads the same float32 values the kernels read.  Never the code under test: host numpy only.

  lists       ragged: row r owns cand[off[r] .. off[r + 1]), scores / priors flat and parallel to cand; shared (off None): one list for
              every row, scores / priors (n, n_cand)
  score       a gather from a float32 matrix (n, n_item): a negative id is padding (-inf); a ragged row whose offsets are negative,
              descending or end beyond n_cand, or that holds an id >= n_item, is rejected (its entries -inf, counted once); a shared
              list with an id >= n_item rejects every row, counted once; an entry no accepted row owns is -inf
  key         t = score, or with a prior (float32)(w_score * float64(score) + w_prior * float64(prior)): two float64 products and one
              float64 sum, each rounded once - numpy's float64 arithmetic, which does not contract
  rerank      selectable = id >= 0 and t neither NaN nor -inf; order = higher t, lower id, lower position; -0.0 and +0.0 are one key,
              written +0.0; the best min(k, selectable) entries, -1 / -inf / -1 behind; count = selectable, not clipped; a ragged row
              with malformed offsets or more than LEN_MAX entries is rejected (all -1, count 0, counted once)"""
import numpy as np

LEN_MAX = 4096
K_MAX = 4096


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids = np.concatenate([np.asarray(l, np.int32) for l in lists]) if len(lists) and off[-1] else np.zeros(0, np.int32)
    return off, ids.astype(np.int32)


def csr_of_padded(mat):
    """An (n, C) matrix padded with -1 as a ragged list with off[r] = r C (the padding stays in the lists)."""
    mat = np.asarray(mat, np.int32)
    return (np.arange(mat.shape[0] + 1, dtype=np.int64) * mat.shape[1]).astype(np.int32), mat.reshape(-1).copy()


def row_span(off, r, n_cand):
    """(o0, o1) of ragged row r, or None when the offsets are negative, descending or end beyond n_cand."""
    o0, o1 = int(off[r]), int(off[r + 1])
    return None if (o0 < 0 or o1 < o0 or o1 > n_cand) else (o0, o1)


def score_lists(full, off, cand):
    """(scores, bad rows): full (n, n_item) float32; off None -> (n, n_cand), else flat (n_cand)."""
    full = np.asarray(full, np.float32)
    n, N = full.shape
    cand = np.asarray(cand, np.int64)
    gather = lambda r, ids: np.where(ids >= 0, full[r, np.clip(ids, 0, N - 1)], np.float32(-np.inf)).astype(np.float32)
    if off is None:
        if len(cand) and cand.max() >= N:
            return np.full((n, len(cand)), -np.inf, np.float32), 1
        return np.stack([gather(r, cand) for r in range(n)]) if n else np.zeros((0, len(cand)), np.float32), 0
    out = np.full(len(cand), -np.inf, np.float32)
    bad = 0
    for r in range(n):
        span = row_span(off, r, len(cand))
        if span is None or (span[1] > span[0] and cand[span[0]:span[1]].max() >= N):
            bad += 1
            continue
        out[span[0]:span[1]] = gather(r, cand[span[0]:span[1]])
    return out, bad


def key_of(score, prior=None, weights=(1.0, 0.0)):
    """The float32 key of every entry; -0.0 folded onto +0.0."""
    t = np.asarray(score, np.float32)
    if prior is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.float64(weights[0]) * t.astype(np.float64) + np.float64(weights[1]) * np.asarray(prior, np.float32).astype(np.float64)).astype(np.float32)
    return t + np.float32(0.0)


def rerank_row(ids, t, k):
    """One list: (ids (k), keys (k), positions (k), count)."""
    ids = np.asarray(ids, np.int64)
    pos = np.nonzero((ids >= 0) & ~np.isnan(t) & ~np.isneginf(t))[0]
    order = pos[np.lexsort((pos, ids[pos], -t[pos].astype(np.float64)))][:k]
    oi, ov, op = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32), np.full(k, -1, np.int32)
    oi[:len(order)] = ids[order]; ov[:len(order)] = t[order]; op[:len(order)] = order
    return oi, ov, op, len(pos)


def rerank(off, cand, n, score, k, prior=None, weights=(1.0, 0.0)):
    """(ids (n, k), keys (n, k), positions (n, k), counts (n), bad rows).  score / prior: flat (ragged) or (n, n_cand) (shared)."""
    cand = np.asarray(cand, np.int64)
    t = key_of(score, prior, weights)
    oi, ov, op = np.full((n, k), -1, np.int32), np.full((n, k), -np.inf, np.float32), np.full((n, k), -1, np.int32)
    cnt = np.zeros(n, np.int32)
    bad = 0
    for r in range(n):
        if off is None:
            row = rerank_row(cand, t[r], k)
        else:
            span = row_span(off, r, len(cand))
            if span is None or span[1] - span[0] > LEN_MAX:
                bad += 1
                continue
            row = rerank_row(cand[span[0]:span[1]], t[span[0]:span[1]], k)
        oi[r], ov[r], op[r], cnt[r] = row
    return oi, ov, op, cnt, bad


def brute_force_row(ids, t, k):
    """The same order through Python's sort on (key, id, position) tuples: a check of `rerank_row` itself."""
    ent = []
    for i, (j, v) in enumerate(zip(ids, t)):
        v = float(v)
        if j < 0 or v != v or v == float("-inf"):
            continue
        ent.append((-(v + 0.0), int(j), i))
    ent.sort()
    return [(j, i) for _, j, i in ent[:k]]
