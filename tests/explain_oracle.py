"""float64 numpy oracle of the leave-one-out attribution (models.GruBasic.explain -> poi_explain_loo): every variant is the oracle's
`predict` on the REDUCED sequence with the bins of the reduced sequence (so the step after a removed check-in is binned against the
check-in before it), scored with test_gpu_session.oracle_scores.  Nothing here knows how the kernel walks."""
import numpy as np

from oracle import poi_oracle as O
from tests.test_gpu_session import oracle_scores, seq_bins


def groups_of(seq, by):
    """(group of every position, the POI every group removes): one group per position, or one per distinct POI by first occurrence."""
    seq = [int(v) for v in seq]
    if by == "checkin":
        return list(range(len(seq))), seq
    order = []
    for v in seq:
        if v not in order:
            order.append(v)
    return [order.index(v) for v in seq], order


def variant_seq(seq, grp, key):
    """The history without the positions of group `key` (key -1: the whole history)."""
    return [int(v) for v, g in zip(seq, grp) if g != key]


def variant_state(P, T, seq, spatial):
    """(h (dim), sts (n_dist + 1) | None, last_poi) of a fresh session advanced through `seq`."""
    seq = list(seq)
    if not seq:
        h = np.zeros(P["wh"].shape[-1])
        if not spatial:
            return h, None, -1
        z = np.asarray(P["bs"], np.float64)
        e = np.exp(z - z.max())
        return h, e / e.sum(), -1
    if spatial:
        h, st = O.spatial_predict(P, P["lt"], P["di"], [seq], [seq_bins(T, seq)], [np.ones(len(seq), int)])
        return h[0], st[0], seq[-1]
    return O.gru_predict(P, P["lt"], [seq], [np.ones(len(seq), int)])[0], None, seq[-1]


def variant_scores(P, T, state, row_list):
    """(scores of the listed POIs (NaN at -1), their distance terms alone) under one state."""
    h, sts, last = state
    geo = sts is not None and last >= 0
    full = oracle_scores(P, T, h[None], sts[None] if geo else None, [last] if geo else None)[0]
    plain = O.score_all(h[None], P["lt"])[0]
    j = np.asarray(row_list)
    at = np.where(j >= 0, j, 0)
    return np.where(j >= 0, full[at], np.nan), np.where(j >= 0, (full - plain)[at], np.nan)


def explain(P, T, seqs, lists, by="checkin", spatial=True):
    """dict(base (n, C), delta (G, C), off (n + 1), keys (G), h (G, dim), sts (G, n_dist + 1) | None, last (G), seqs: the reduced
    histories, base_geo (n, C) / var_geo (G, C): the distance terms alone)."""
    base, delta, off, keys, hs, ss, ls, red, bgeo, vgeo = [], [], [0], [], [], [], [], [], [], []
    for seq, row_list in zip(seqs, lists):
        grp, kpoi = groups_of(seq, by)
        b, bg = variant_scores(P, T, variant_state(P, T, variant_seq(seq, grp, -1), spatial), row_list)
        base.append(b); bgeo.append(bg)
        for g, poi in enumerate(kpoi):
            r = variant_seq(seq, grp, g)
            st = variant_state(P, T, r, spatial)
            s, sg = variant_scores(P, T, st, row_list)
            delta.append(b - s); vgeo.append(sg); keys.append(poi); hs.append(st[0]); ss.append(st[1]); ls.append(st[2]); red.append(r)
        off.append(len(delta))
    C = np.asarray(lists).shape[1]
    arr = lambda rows, w: np.array(rows, np.float64).reshape(len(rows), w)
    return dict(base=arr(base, C), delta=arr(delta, C), off=np.array(off), keys=np.array(keys, np.int64), h=arr(hs, P["wh"].shape[-1]),
                sts=arr(ss, T["n_dist"] + 1) if spatial else None, last=np.array(ls, np.int64), seqs=red, base_geo=arr(bgeo, C), var_geo=arr(vgeo, C))


def rebinned(T, seqs):
    """(changed, cases): over every middle check-in t of every history, does removing it change the bin of position t + 1?"""
    changed = cases = 0
    for s in seqs:
        s = [int(v) for v in s]
        for t in range(1, len(s) - 1):
            cases += 1
            changed += int(seq_bins(T, [s[t - 1], s[t + 1]])[1] != seq_bins(T, [s[t], s[t + 1]])[1])
    return changed, cases
