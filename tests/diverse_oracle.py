"""float64 numpy oracle of the diversified recommendation (poi_diverse_pool / poi_diverse_rerank / poi_diverse_topk,
models.compute_sub_topk_diverse): the pool from near_oracle's top-k over the finite-scored candidates, the sin^2 Haversine distance,
and the greedy re-ranking with its running maximum of similarities.  Never the code under test: host numpy only."""
import numpy as np

from poi_amd import data
from tests import near_oracle as NO


def pool(sc, mask, m):
    """(ids (n, m) with -1 fill, scores with -inf fill, counts = |C(r)|): the best m candidates by descending score, ties by ascending
    id; NaN and +-inf scores are never pooled (they still count as candidates)."""
    sc = np.asarray(sc, np.float64)
    ids, val, _ = NO.topk(sc, mask & np.isfinite(sc), m)
    return ids, val, mask.sum(axis=1)


def dist_km(coords, a, b):
    """Great-circle distance (km) between the POIs a and b (arrays of ids, broadcast): 12742 asin(min(1, sqrt(sin^2(dlat pi/360) +
    cos(lat_a) cos(lat_b) sin^2(dlon pi/360)))), cos(lat) from data.cos_lat."""
    xy = np.asarray(coords, np.float64)
    cphi = data.cos_lat(xy)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    sa = np.sin((xy[a, 0] - xy[b, 0]) * (np.pi / 360.0))
    sb = np.sin((xy[a, 1] - xy[b, 1]) * (np.pi / 360.0))
    return 12742.0 * np.arcsin(np.minimum(1.0, np.sqrt(sa * sa + cphi[a] * cphi[b] * (sb * sb))))


def pool_size(pool_idx):
    """m per row: the entries before the first -1."""
    neg = np.asarray(pool_idx) < 0
    return np.where(neg.any(axis=1), neg.argmax(axis=1), neg.shape[1])


def similarity(ids, l, items, coords, geo_weight, scale_km):
    """sim(i, l) of every pool member ids[i] against the member ids[l]; a part with zero weight is not evaluated."""
    sim = np.zeros(len(ids))
    if geo_weight > 0.0:
        sim = geo_weight * np.exp(-dist_km(coords, ids, ids[l]) / scale_km)
    if geo_weight < 1.0:
        x = np.asarray(items, np.float64)[ids]
        nrm = np.sqrt((x * x).sum(axis=1))
        den = nrm * nrm[l]
        with np.errstate(invalid="ignore", divide="ignore"):
            emb = np.where(den == 0.0, 0.0, (x @ x[l]) / den)
        sim = sim + (1.0 - geo_weight) * emb if geo_weight > 0.0 else (1.0 - geo_weight) * emb
    return sim


def rerank(pool_idx, pool_score, items, coords, k, trade, geo_weight, scale_km):
    """(idx (n, k) -1 fill, pos (n, k) -1 fill, obj (n, k) -inf fill, min_gap (n)): the greedy MMR selection of include/poi_hip.h.
    min_gap[r] is the smallest difference between the best and the second-best objective over the steps t >= 1 with at least two
    unselected entries (+inf when there is no such step): a float64 kernel must reproduce the picks of a row whose min_gap is clear."""
    pool_idx = np.asarray(pool_idx, np.int64)
    pool_score = np.asarray(pool_score, np.float64)
    n = len(pool_idx)
    idx, pos = np.full((n, k), -1, np.int64), np.full((n, k), -1, np.int64)
    obj, min_gap = np.full((n, k), -np.inf), np.full(n, np.inf)
    ms = pool_size(pool_idx)
    for r in range(n):
        m = int(ms[r])
        if m == 0:
            continue
        ids, s = pool_idx[r, :m], pool_score[r, :m]
        den = s[0] - s[m - 1]
        rel = np.ones(m) if den == 0.0 else (s - s[m - 1]) / den
        pen = np.zeros(m)
        taken = np.zeros(m, bool)
        for t in range(min(k, m)):
            o = trade * rel - (1.0 - trade) * pen
            if t == 0:
                w = 0
            else:
                live = np.nonzero(~taken)[0]
                order = live[np.lexsort((live, -o[live]))]
                w = int(order[0])
                if len(order) > 1:
                    min_gap[r] = min(min_gap[r], o[order[0]] - o[order[1]])
            idx[r, t], pos[r, t], obj[r, t] = ids[w], w, o[w]
            taken[w] = True
            if trade != 1.0 and t + 1 < min(k, m):
                sim = similarity(ids, w, items, coords, geo_weight, scale_km)
                pen = sim if t == 0 else np.maximum(pen, sim)
    return idx, pos, obj, min_gap
