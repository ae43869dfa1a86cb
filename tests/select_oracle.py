"""Numpy oracle of the candidate selection (include/poi_hip.h, poi_topk_select): the definition applied to a given float32 score matrix.
Exact, no tolerance: it reads the same float32 values the kernel reads.  Never the code under test: host numpy only.

  C(r)        = [0, n_item) minus the row's exclusion list
  selectable  = an entry of C(r) whose score is neither NaN nor -inf (+inf is selectable)
  result      = the best min(k, |selectable|) entries, higher score first, then the lower id; -0.0 and +0.0 are the same score and
                come out as +0.0; -1 ids and -inf scores behind; count = |C(r)|; a row whose list is not ascending or leaves
                [0, n_item) is rejected (all -1, count 0)."""
import numpy as np

K_MAX = 4096


def fold(sc):
    """float32 scores with -0.0 folded onto +0.0 (x + 0.0 is +0.0 for both zeros under round-to-nearest)."""
    return np.asarray(sc, np.float32) + np.float32(0.0)


def bad_list(lst, n_item):
    lst = np.asarray(lst, np.int64)
    return bool(len(lst) and (lst.min() < 0 or lst.max() >= n_item or np.any(np.diff(lst) <= 0)))


def select(sc, k, ex_off=None, ex=None):
    """(ids (n, k) int32, scores (n, k) float32, counts (n) int32, bad rows) of the float32 matrix sc (n, n_item)."""
    sc = fold(sc)
    n, N = sc.shape
    ids = np.full((n, k), -1, np.int32)
    val = np.full((n, k), -np.inf, np.float32)
    cnt = np.zeros(n, np.int32)
    bad = 0
    for r in range(n):
        mask = np.ones(N, bool)
        if ex_off is not None:
            lst = np.asarray(ex[ex_off[r]:ex_off[r + 1]], np.int64) if ex_off[r + 1] >= ex_off[r] >= 0 else None
            if lst is None or bad_list(lst, N):
                bad += 1
                continue
            mask[lst] = False
        cnt[r] = mask.sum()
        s = sc[r]
        cand = np.nonzero(mask & ~np.isnan(s) & ~np.isneginf(s))[0]
        order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))][:k]      # (float64: the negation of a float32 is exact either way)
        ids[r, :len(order)] = order
        val[r, :len(order)] = s[order]
    return ids, val, cnt, bad


def brute_force(sc, k, ex_off=None, ex=None):
    """The same definition through Python's sort on (score, id) tuples, one row at a time: a check of `select` itself."""
    sc = np.asarray(sc, np.float32)
    out = []
    for r in range(sc.shape[0]):
        gone = set() if ex_off is None else set(int(j) for j in ex[ex_off[r]:ex_off[r + 1]])
        ent = []
        for j in range(sc.shape[1]):
            v = float(sc[r, j])
            if j in gone or v != v or v == float("-inf"):
                continue
            ent.append((-(v + 0.0), j))
        ent.sort()
        out.append([j for _, j in ent[:k]])
    return out


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids = np.concatenate([np.asarray(l, np.int32) for l in lists]) if len(lists) and off[-1] else np.zeros(0, np.int32)
    return off, ids.astype(np.int32)
