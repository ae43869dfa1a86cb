"""float64 numpy oracle of the restricted recommendation (poi_score_topk_near, models.compute_sub_topk_near): candidate masks from the
exact predicate of data.fpmc_neighbors_host, scores from the float32-rounded tables through oracle.poi_oracle, top-k by descending
score then ascending id with a -1 fill.  Never the code under test: host numpy only."""
import math

import numpy as np

from oracle import poi_oracle as O
from poi_amd import data

DEG = 0.017453292519943295


def haversine_rows(coords, anchor):
    """c(anchor[r], j) for every row and POI in cal_dis's operation order (cos of the latitudes from data.cos_lat)."""
    xy = np.asarray(coords, np.float64)
    cphi = data.cos_lat(xy)
    a = np.asarray(anchor, np.int64)
    la, lo = xy[a, 0][:, None], xy[a, 1][:, None]
    return (1.0 - np.cos((la - xy[None, :, 0]) * DEG)) / 2 + cphi[a][:, None] * cphi[None, :] * (1.0 - np.cos((lo - xy[None, :, 1]) * DEG)) / 2


def candidate_mask(coords, anchor, within_km, ex_off=None, ex=None):
    """(n, n_item) bool: j is a candidate of row r <=> (anchor[r] < 0 or no radius or c(anchor[r], j) < c_r or j == anchor[r]) and j is
    not on the row's exclusion list.  c < c_r with c_r = data.ud_threshold: the predicate of data.fpmc_neighbors_host, and like there
    every pair within 1e-9 (relative) of the threshold is recomputed with the scalar math.cos of the reference."""
    xy = np.asarray(coords, np.float64)
    anchor = np.asarray(anchor, np.int64)
    n, N = len(anchor), len(xy)
    mask = np.ones((n, N), bool)
    c_r = np.inf if within_km is None else data.ud_threshold(within_km)
    rows = np.nonzero(anchor >= 0)[0]
    if np.isfinite(c_r) and len(rows):
        cphi = data.cos_lat(xy)
        c = haversine_rows(xy, anchor[rows])
        for q, k in zip(*np.nonzero(np.abs(c - c_r) <= 1e-9 * c_r)):
            i = int(anchor[rows[q]])
            c[q, k] = (1.0 - math.cos((xy[i, 0] - xy[k, 0]) * DEG)) / 2 + cphi[i] * cphi[k] * (1.0 - math.cos((xy[i, 1] - xy[k, 1]) * DEG)) / 2
        mask[rows] = c < c_r
        mask[rows, anchor[rows]] = True
    if ex_off is not None:
        for r in range(n):
            mask[r, np.asarray(ex[ex_off[r]:ex_off[r + 1]], np.int64)] = False
    return mask


def brute_force_mask(coords, anchor, within_km):
    """cal_dis(anchor[r], j) <= within_km, one scalar libm call chain per pair (public/Load_Data_fpmc_lr.py:25-34)."""
    xy = np.asarray(coords, np.float64)
    out = np.zeros((len(anchor), len(xy)), bool)
    for r, i in enumerate(anchor):
        for k in range(len(xy)):
            a, b = (xy[i, 0] - xy[k, 0]) * DEG, (xy[i, 1] - xy[k, 1]) * DEG
            c = (1.0 - math.cos(a)) / 2 + math.cos(xy[i, 0] * DEG) * math.cos(xy[k, 0] * DEG) * (1.0 - math.cos(b)) / 2
            out[r, k] = 12742 * math.asin(math.sqrt(c)) <= within_km
    return out


def scores(users, items, anchor=None, wd=None, sts=None, coords=None, dd_m=None, n_dist=None):
    """float64 scores of every POI: users . items[:-1]^T, plus wd * sts[bin(anchor, .)] for bins below n_dist on rows with an anchor."""
    sc = O.score_all(np.asarray(users, np.float64), np.asarray(items, np.float64))
    if wd is not None:
        anchor = np.asarray(anchor, np.int64)
        c = np.asarray(coords, np.float64)
        ul = np.stack([data.cal_dis_vec(c[max(l, 0), 0], c[max(l, 0), 1], c[:, 0], c[:, 1], dd_m, n_dist) for l in anchor])
        sc = sc + wd * O.acquire_prob(np.asarray(sts, np.float64), ul, n_dist) * (anchor >= 0)[:, None]
    return sc


def topk(sc, mask, k):
    """(ids (n, k) with -1 fill, scores with -inf fill, counts): the candidates by descending score, ties by ascending id."""
    n = len(sc)
    ids, val = np.full((n, k), -1, np.int64), np.full((n, k), -np.inf)
    for r in range(n):
        cand = np.nonzero(mask[r])[0]
        order = cand[np.lexsort((cand, -sc[r, cand]))][:k]
        ids[r, :len(order)] = order
        val[r, :len(order)] = sc[r, order]
    return ids, val, mask.sum(axis=1)


def qualifying(sc, mask, k):
    """Rows whose top-(k + 1) adjacent gaps AMONG THE CANDIDATES are >= 1e-6 max|score| (the rule of tests/test_gpu_session.py): a float32
    kernel must rank them exactly."""
    lim = 1e-6 * np.abs(sc).max()
    ok = np.ones(len(sc), bool)
    for r in range(len(sc)):
        top = -np.sort(-sc[r, mask[r]])[:k + 1]
        ok[r] = len(top) < 2 or np.diff(-top).min() >= lim
    return ok
