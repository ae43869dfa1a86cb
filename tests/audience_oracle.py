"""float64 numpy oracle of the audience recommendation (poi_score_audience / poi_audience_rows, models.recommend_audience): the score
matrix of tests/near_oracle.py::scores TRANSPOSED - a row per POI, a column per user - and the selection of the same module
(NO.topk / NO.qualifying) over the user axis.  Never the code under test: host numpy only."""
import numpy as np

from tests import near_oracle as NO

topk = NO.topk                # (sc (n_q, n), mask, k) -> (ids with -1 fill, scores with -inf fill, counts)
qualifying = NO.qualifying    # queries whose top-(k + 1) gaps among the candidates are >= 1e-6 max|score|


def scores_t(users, items, last=None, term=None, T=None):
    """(n_item, n) float64: s(u, j) of every POI j (row) for every candidate row u (column).  term = (wd, sts) with last (the rows' last
    POI, -1: no distance term) and T (coords, dd_m, n_dist), or None."""
    if term is None:
        return NO.scores(users, items).T.copy()
    return NO.scores(users, items, last, term[0], term[1], T["coords"], T["dd_m"], T["n_dist"]).T.copy()


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, (np.concatenate([np.asarray(l, np.int64) for l in lists]) if len(lists) and off[-1] else np.zeros(0, np.int64))


def visitor_sets(seqs, n_item):
    """Per POI the set of users whose train sequence holds it (ids >= n_item are padding: no visit)."""
    out = [set() for _ in range(n_item)]
    for u, s in enumerate(seqs):
        for j in s:
            if 0 <= int(j) < n_item:
                out[int(j)].add(u)
    return out


def visitor_lists(seqs, n_item, pois, segment=None):
    """CSR (off, rows) of the queries' train visitors, ascending; with `segment` (ascending user ids) restricted to it and re-indexed."""
    vs = visitor_sets(seqs, n_item)
    pos = None if segment is None else {int(u): i for i, u in enumerate(segment)}
    lists = []
    for j in pois:
        us = sorted(vs[int(j)])
        lists.append(us if pos is None else [pos[u] for u in us if u in pos])
    return csr(lists)


def candidate_mask(n_q, n, ex_off=None, ex=None):
    """(n_q, n) bool: row u is a candidate of query q unless it stands on the query's list."""
    mask = np.ones((n_q, n), bool)
    if ex_off is not None:
        for q in range(n_q):
            mask[q, np.asarray(ex[ex_off[q]:ex_off[q + 1]], np.int64)] = False
    return mask


def brute_force(users, items, pois, k, excluded=None):
    """The definition, one pair at a time: python floats, one sort per query.  excluded: per query a set of rows, or None."""
    users, items = np.asarray(users, np.float64), np.asarray(items, np.float64)
    ids, cnt = [], []
    for qi, j in enumerate(pois):
        cand = [u for u in range(len(users)) if excluded is None or u not in excluded[qi]]
        sc = {u: float(sum(float(a) * float(b) for a, b in zip(users[u], items[j]))) for u in cand}
        order = sorted(cand, key=lambda u: (-sc[u], u))[:k]
        ids.append(order + [-1] * (k - len(order)))
        cnt.append(len(cand))
    return np.array(ids, np.int64), np.array(cnt, np.int64)
