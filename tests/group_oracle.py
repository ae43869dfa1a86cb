"""float64 numpy oracle of the group recommendation (poi_group_topk / poi_group_topk_scores, models.recommend_group): member scores from
tests/near_oracle.py (the anchor is the member's last POI), the aggregate over each group's list, the candidate mask from the group's
exclusion list, then near_oracle's top-k (descending aggregate, ascending id, -1 fill) and its qualifying rule.  Never the code under
test: host numpy only."""
import numpy as np

from tests import near_oracle as NO

AGGS = ("mean", "min")


def member_scores(users, items, last_poi=None, wd=None, sts=None, coords=None, dd_m=None, n_dist=None):
    """(n, n_item) float64: users . items[:-1]^T, plus wd * sts[bin(last_poi, .)] for bins below n_dist on rows with last_poi >= 0."""
    return NO.scores(users, items, last_poi, wd, sts, coords, dd_m, n_dist)


def csr(groups):
    """list of id lists -> (off int64, ids int64)."""
    off = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=off[1:])
    return off, (np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) and off[-1] else np.zeros(0, np.int64))


def aggregate(sc, off, ids, agg):
    """(n_grp, n_item) float64: the mean or the minimum of the members' score rows; a member listed twice counts twice; an empty
    group's row is zero (it has no candidates)."""
    assert agg in AGGS
    out = np.zeros((len(off) - 1, sc.shape[1]))
    for g in range(len(off) - 1):
        rows = sc[np.asarray(ids[off[g]:off[g + 1]], np.int64)]
        if len(rows):
            out[g] = rows.sum(axis=0) / len(rows) if agg == "mean" else rows.min(axis=0)
    return out


def candidate_mask(off, n_item, ex_off=None, ex=None):
    """(n_grp, n_item) bool: every POI that is not on the group's exclusion list; an empty group has no candidates."""
    mask = np.ones((len(off) - 1, n_item), bool)
    mask[np.diff(off) == 0] = False
    if ex_off is not None:
        for g in range(len(off) - 1):
            mask[g, np.asarray(ex[ex_off[g]:ex_off[g + 1]], np.int64)] = False
    return mask


def topk(agg_sc, mask, k):
    return NO.topk(agg_sc, mask, k)


def qualifying(agg_sc, mask, k):
    return NO.qualifying(agg_sc, mask, k)
