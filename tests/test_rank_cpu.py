"""CPU tests of the exact target rank's host side: the oracle (tests/rank_oracle.py) against the position of the target in a full
top-K list, the declarations of the two entry points (header, ctypes binding, build list) and the formulas of
evaluate.full_rank_metrics against evaluate.rank_metrics.  No GPU."""
import os
import re

import numpy as np

from oracle import poi_oracle as O
from poi_amd import evaluate as E
from tests import rank_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _position(sc, t):
    return [int(np.nonzero(O.topk_desc(sc[r:r + 1], sc.shape[1])[0] == t[r])[0][0]) for r in range(len(t))]


def test_oracle_rank_is_the_position_in_a_full_list():
    rng = np.random.default_rng(1)
    sc = rng.normal(size=(12, 97))
    tgt = rng.integers(0, 97, (12, 3))
    out = RO.ranks(sc, tgt, np.ones_like(tgt))
    for i in range(3):
        assert out["rank"][:, i].tolist() == _position(sc, tgt[:, i])
    assert (out["count"] == 97).all() and (out["a"] == 0).mean() > 0.9
    assert np.array_equal(out["score"], np.take_along_axis(sc, tgt, 1))


def test_oracle_rank_with_planted_exact_ties():
    rng = np.random.default_rng(2)
    sc = rng.normal(size=(6, 40))
    tgt = rng.integers(0, 40, (6, 1))
    for r in range(6):                                   # copies of the target's score below and above its id
        for j in rng.choice(40, 5, replace=False):
            sc[r, j] = sc[r, tgt[r, 0]]
    out = RO.ranks(sc, tgt, np.ones_like(tgt))
    assert out["rank"][:, 0].tolist() == _position(sc, tgt[:, 0])
    assert (out["a"][:, 0] >= 4).all()                   # the copies sit inside the gap band
    assert ((out["greater_clear"] <= out["rank"]) & (out["rank"] <= out["greater_clear"] + out["a"])).all()


def test_oracle_mask_exclusion_and_range():
    sc = np.array([[5.0, 1.0, 3.0, 3.0, 4.0]])
    tgt = np.array([[3, 2, 0, 5, -1, 1]]); tm = np.array([[1, 1, 1, 1, 1, 0]])
    out = RO.ranks(sc, tgt, tm)
    assert out["rank"].tolist() == [[3, 2, 0, -1, -1, -1]] and out["count"].tolist() == [5]
    out = RO.ranks(sc, tgt, tm, np.array([0, 2]), np.array([0, 2]))       # POIs 0 and 2 leave the ranking
    assert out["rank"].tolist() == [[1, -1, -1, -1, -1, -1]] and out["count"].tolist() == [3]


def test_entry_points_are_declared_bound_and_built():
    import poi_amd
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    for name in ("poi_score_rank", "poi_rank_scores"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/poi_hip.h" % name
        assert name in poi_amd._lib.SIGNATURES, "%s has no ctypes binding" % name
        assert len(poi_amd._lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, "%s: the binding's argument count differs from the header's" % name
    assert "rank.hip" in poi_amd.build.SOURCES
    assert "rank_splits" in poi_amd._lib.PLAN_KEYS
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr)
    assert hasattr(poi_amd.models._Base, "compute_sub_target_rank") and hasattr(poi_amd.models.Session, "rank_of")
    assert hasattr(E, "full_rank_metrics")


def test_rank_summary_agrees_with_rank_metrics():
    rng = np.random.default_rng(3)
    n, N, lt = 50, 60, 3
    sc = rng.normal(size=(n, N))
    tgt = np.stack([rng.choice(N, lt, replace=False) for _ in range(n)])
    tm = (rng.random((n, lt)) < 0.7).astype(int); tm[:, 0] = 1
    out = RO.ranks(sc, tgt, tm)
    at = [1, 5, 10, 20]
    got = E.rank_summary(out["rank"], out["count"], at)
    want = E.rank_metrics(O.topk_desc(sc, 20), tgt, tm, at)
    also = E.rank_metrics(RO.rank_list(out["rank"], tgt, 20), tgt, tm, at)
    for k in at:
        for key in ("hits", "recall", "ndcg"):
            assert abs(got["at"][k][key] - want[k][key]) < 1e-12, (k, key)
            assert abs(got["at"][k][key] - also[k][key]) < 1e-12, (k, key)
    ref = RO.summary(out["rank"], out["count"])
    for key in ("mrr", "mean_rank", "auc_full"):
        assert abs(got[key] - ref[key]) < 1e-12, key
    r = np.sort(out["rank"][out["rank"] >= 0])
    assert got["median_rank"] == r[(len(r) - 1) // 2] and got["n"] == tm.sum()
