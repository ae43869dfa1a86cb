"""float64 numpy oracle of the similar-rows entries (poi_row_inv_norms / poi_similar_topk / poi_similar_rows / poi_similar_nearest,
models.similar_pois / similar_users / nearest_visited): the full similarity matrix from tests/diverse_oracle.py::dist_km and float64
cosines, the selection of tests/near_oracle.py (topk / qualifying) over it, and the nearest-visited arg-max with its best-to-second
gap.  Never the code under test: host numpy only."""
import math

import numpy as np

from tests import audience_oracle as AO
from tests import diverse_oracle as DO
from tests import near_oracle as NO

topk = NO.topk                # (sim (n_q, n), mask, k) -> (ids with -1 fill, sims with -inf fill, counts)
qualifying = NO.qualifying    # queries whose top-(k + 1) gaps among the candidates are >= 1e-6 max|sim|
csr = AO.csr


def inv_norms(x):
    """1 / |x_i| in float64, 0 for a zero row."""
    s = (np.asarray(x, np.float64) ** 2).sum(axis=1)
    with np.errstate(divide="ignore"):
        return np.where(s == 0.0, 0.0, 1.0 / np.sqrt(s))


def cosines(x):
    """(n, n) float64 cosines of the rows, 0 where either row is zero."""
    x = np.asarray(x, np.float64)
    nrm = np.sqrt((x * x).sum(axis=1))
    den = nrm[:, None] * nrm[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0.0, 0.0, (x @ x.T) / den)


def sim_matrix(x, coords=None, g=0.0, scale_km=1.0):
    """(n, n) float64: g exp(-d / scale_km) + (1 - g) cos; a part with zero weight is not evaluated."""
    emb = cosines(x)
    if g == 0.0:
        return emb
    n = len(emb)
    i = np.arange(n)
    geo = np.exp(-DO.dist_km(np.asarray(coords)[:n], i[:, None], i[None, :]) / scale_km)
    return g * geo + (1.0 - g) * emb


def candidate_mask(queries, n, ex_off=None, ex=None):
    """(n_q, n) bool: row j is a candidate of query q unless it is the query's own row or stands on the query's list."""
    mask = AO.candidate_mask(len(queries), n, ex_off, ex)
    mask[np.arange(len(queries)), np.asarray(queries, np.int64)] = False
    return mask


def brute_force(x, coords, g, scale_km, queries, k, excluded=None):
    """The definition, one pair at a time: python floats and math, one sort per query.  excluded: per query a set of rows, or None."""
    x = np.asarray(x, np.float64)
    n = len(x)
    nrm = [math.sqrt(sum(float(v) * float(v) for v in row)) for row in x]

    def sim(i, j):
        dot = sum(float(a) * float(b) for a, b in zip(x[i], x[j]))
        emb = 0.0 if nrm[i] == 0.0 or nrm[j] == 0.0 else dot / (nrm[i] * nrm[j])
        if g == 0.0:
            return emb
        (la, lo), (lb, lp) = coords[i], coords[j]
        sa, sb = math.sin((la - lb) * math.pi / 360.0), math.sin((lo - lp) * math.pi / 360.0)
        h = sa * sa + math.cos(la * math.pi / 180.0) * math.cos(lb * math.pi / 180.0) * sb * sb
        return g * math.exp(-12742.0 * math.asin(min(1.0, math.sqrt(h))) / scale_km) + (1.0 - g) * emb
    ids, val, cnt = [], [], []
    for qi, q in enumerate(queries):
        cand = [j for j in range(n) if j != q and (excluded is None or j not in excluded[qi])]
        sc = {j: sim(q, j) for j in cand}
        order = sorted(cand, key=lambda j: (-sc[j], j))[:k]
        ids.append(order + [-1] * (k - len(order)))
        val.append([sc[j] for j in order] + [-np.inf] * (k - len(order)))
        cnt.append(len(cand))
    return np.array(ids, np.int64), np.array(val), np.array(cnt, np.int64)


def nearest(lists, h_off, h_ids, items, coords, g, scale_km):
    """(pos (n, k) -1 fill, sim (n, k) -inf fill, gap (n, k), twin (n, k) bool): per listed POI the history POSITION with the largest
    similarity (tests/diverse_oracle.py::similarity's formulas), ties to the lower position; gap = best minus the best of the OTHER
    positions (+inf with fewer than two); twin: the runner-up ties exactly and holds the same POI as the best."""
    lists = np.asarray(lists, np.int64)
    n, k = lists.shape
    pos, sim = np.full((n, k), -1, np.int64), np.full((n, k), -np.inf)
    gap, twin = np.full((n, k), np.inf), np.zeros((n, k), bool)
    for r in range(n):
        h = np.asarray(h_ids[h_off[r]:h_off[r + 1]], np.int64)
        if not len(h):
            continue
        for i in range(k):
            j = lists[r, i]
            if j < 0:
                continue
            ids = np.concatenate(([j], h))
            s = DO.similarity(ids, 0, items, coords, g, scale_km)[1:]
            w = int(np.argmax(s))                    # (the first of the maxima)
            pos[r, i], sim[r, i] = w, s[w]
            if len(h) > 1:
                rest = np.delete(s, w)
                at = int(np.argmax(rest))
                gap[r, i] = s[w] - rest[at]
                twin[r, i] = rest[at] == s[w] and np.delete(h, w)[at] == h[w]
    return pos, sim, gap, twin


def covisit_share(voff, vus, a, b):
    """The share of the pairs (a[i], b[i]) of POIs that share at least one visitor, from the visitor CSR (voff, vus): sets, one pair at
    a time."""
    sets = [set(np.asarray(vus[voff[j]:voff[j + 1]]).tolist()) for j in range(len(voff) - 1)]
    hit = [bool(sets[int(i)] & sets[int(j)]) for i, j in zip(a, b)]
    return float(np.mean(hit)) if hit else 0.0
