"""CPU tests of the leave-one-out attribution's host side: header / export / binding agreement with the ABI still 9, the group and
column builders of models.py (torch ops) against a plain Python loop, the oracle of tests/explain_oracle.py against `predict` on the
whole sequence, the host argument refusals of models.Explainer, and evaluate.attribution_by_recency on a hand-made model.
No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import poi_amd
from oracle import poi_oracle as O
from poi_amd import evaluate as E, models as M
from tests import explain_oracle as XO
from tests.test_gpu_session import geo_problem, seq_bins, seqs_of, spatial_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_bindings_agree_and_the_abi_is_still_9():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    abi = open(os.path.join(poi_amd.build.CSRC, "abi_serve.hip")).read()
    m = re.search(r"\bint poi_explain_loo\(([^;]*?)\);", hdr, re.S)
    assert m, "poi_explain_loo is not declared in include/poi_hip.h"
    d = re.search(r"\nint poi_explain_loo\(([^{]*?)\) \{", abi, re.S)
    assert d, "poi_explain_loo is not defined in csrc/abi_serve.hip"
    assert len(poi_amd._lib.SIGNATURES["poi_explain_loo"][1]) == m.group(1).count(",") + 1 == d.group(1).count(",") + 1 == 25
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    assert hdr.index("additive to 9: leave-one-out attribution") < hdr.index("#define POI_ABI_VERSION 9")
    assert "explain.hip" in poi_amd.build.SOURCES and os.path.exists(os.path.join(poi_amd.build.CSRC, "explain.hip"))
    options = open(os.path.join(poi_amd.build.CSRC, "abi.hip")).read()
    for key in ("explain_columns", "explain_tiles", "explain_start"):
        assert key in poi_amd._lib.PLAN_KEYS and '"%s"' % key in hdr and '{"%s", &poi_ctx::LastPlan::%s}' % (key, key) in options
    assert '{"explain_start", &c->explain_start, 0, 1}' in options
    for name in ("explain_base", "explain_walk"):
        assert '"%s"' % name in hdr and '"%s"' % name in open(os.path.join(poi_amd.build.CSRC, "explain.hip")).read()


def _loop_groups(seqs, by):
    grp, g_off, keys, first, row = [], [0], [], [], []
    for r, s in enumerate(seqs):
        seen = []
        for t, v in enumerate(s):
            if by == "checkin" or v not in seen:
                seen.append(v if by == "poi" else t)
                keys.append(v); first.append(t); row.append(r)
            grp.append(seen.index(v) if by == "poi" else t)
        g_off.append(len(keys))
    return grp, g_off, keys, first, row


@pytest.mark.parametrize("by", ["checkin", "poi"])
def test_groups_and_columns_against_a_plain_loop(by):
    rng = np.random.default_rng(5)
    seqs = [list(rng.integers(0, 9, L)) for L in (0, 1, 50, 17, 16, 33, 2, 0, 48, 5, 49, 3)]
    seqs[3][16] = seqs[3][2]                                   # a POI whose first visit lies before a checkpoint, a later one behind it
    seqs[6] = [4, 4]                                           # a consecutive repeat: one group under by="poi"
    off = torch.as_tensor(np.r_[0, np.cumsum([len(s) for s in seqs])].astype(np.int64))
    p = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]))
    grp, g_off, keys, first, row = M.explain_groups(off, p, by)
    want = _loop_groups(seqs, by)
    for got, w in zip((grp, g_off, keys, first, row), want):
        assert got.tolist() == [int(v) for v in w]
    if by == "poi":
        assert g_off[7] - g_off[6] == 1 and g_off[1] == 0 and g_off[-1] < len(p)
    lens = off[1:] - off[:-1]
    for mode in (1, 0):
        base, var = M.explain_columns(lens, g_off, first, row, mode)
        assert base.dtype == var.dtype == torch.int32 and base.shape == (len(seqs), 4) and var.shape == (len(want[2]), 4)
        L = [len(s) for s in seqs]
        assert base[:, 0].tolist() == sorted(range(len(seqs)), key=lambda r: -L[r]) and set(base[:, 1].tolist()) == {-1} and not base[:, 2:].any()
        cols = []
        for g, (f, r) in enumerate(zip(want[3], want[4])):
            start = 16 * (f // 16) if mode else 0
            cols.append((r, g - want[1][r], start, 0))
        cols.sort(key=lambda c: -(L[c[0]] - c[2]))             # stable: equal remaining walks keep their order
        assert [tuple(c) for c in var.tolist()] == cols
        rem = [L[c[0]] - c[2] for c in var.tolist()]
        assert rem == sorted(rem, reverse=True)
        top = max(c[2] for c in cols)                          # check-ins start as late as 48; the 9 distinct POIs all occur by position 32
        assert top == (0 if mode == 0 else 48 if by == "checkin" else 16 * (max(want[3]) // 16)) and (mode == 0 or top >= 16)
    with pytest.raises(ValueError, match="by must be"):
        M.explain_groups(off, p, "user")


def test_oracle_base_variant_is_predict_on_the_whole_sequence():
    T = geo_problem(101, n_user=24, n_item=50, n_dist=11, dim=8, len_min=1, len_max=12)
    P = spatial_init(101, T)
    seqs = seqs_of(T)
    for s in seqs[:6]:
        grp, keys = XO.groups_of(s, "checkin")
        assert XO.variant_seq(s, grp, -1) == [int(v) for v in s] and keys == [int(v) for v in s]
        h, st, last = XO.variant_state(P, T, XO.variant_seq(s, grp, -1), True)
        hw, sw = O.spatial_predict(P, P["lt"], P["di"], [list(s)], [seq_bins(T, s)], [np.ones(len(s), int)])
        assert np.array_equal(h, hw[0]) and np.array_equal(st, sw[0]) and last == s[-1]
    s = [3, 7, 3, 3, 9]
    grp, keys = XO.groups_of(s, "poi")
    assert grp == [0, 1, 0, 0, 2] and keys == [3, 7, 9] and XO.variant_seq(s, grp, 0) == [7, 9] and XO.variant_seq(s, grp, 1) == [3, 3, 3, 9]
    lists = np.array([[1, -1, 4]])
    R = XO.explain(P, T, [seqs[0]], lists)
    assert R["delta"].shape == (len(seqs[0]), 3) and np.isnan(R["base"][0, 1]) and np.isnan(R["delta"][:, 1]).all()
    assert np.abs(R["delta"][:, [0, 2]]).max() > 0 and R["off"].tolist() == [0, len(seqs[0])]


def _bare(cls, **attrs):
    obj = object.__new__(cls)
    obj.__dict__.update(dict(device="cpu", n_item=50, n_user=4, kdim=64, dim=64, coords=None), **attrs)
    return obj


def test_host_argument_refusals():
    m = M.Explainer(_bare(M.OboGru))
    assert m._explain_lists([[1, -1, 3]], 1).tolist() == [[1, -1, 3]]
    with pytest.raises(ValueError, match="1 <= C <= 32"):
        m._explain_lists(np.zeros((2, 33), int), 2)
    with pytest.raises(ValueError, match="2 rows"):
        m._explain_lists(np.zeros((3, 4), int), 2)
    for bad in ([[50]], [[-2]]):
        with pytest.raises(IndexError, match="listed POIs"):
            m._explain_lists(bad, 1)
    with pytest.raises(ValueError, match="by must be"):
        m.explain([0], [[1]], by="user")
    for cls in (M.Lstm, M.Rnn, M.OboCARNN):
        with pytest.raises(poi_amd._lib.PoiError, match="out of scope"):
            M.Explainer(_bare(cls))
    with pytest.raises(poi_amd._lib.PoiError, match="out of scope"):
        M.Explainer(object())
    with pytest.raises(poi_amd._lib.PoiError, match="coords="):
        M.Explainer(_bare(M.OboSpatialGru))
    with pytest.raises(poi_amd._lib.PoiError, match="pad_dim"):
        M.Explainer(_bare(M.OboGru, kdim=20))


class _Toy:
    """What evaluate.attribution_by_recency reads: compute_sub_topk of the model and an explain callable."""
    n_item = 9
    _lens = [3, 1, 0, 2]

    def compute_sub_topk(self, se, k):
        return torch.as_tensor(np.tile(np.arange(k, dtype=np.int32), (len(se), 1)))

    def explain(self, se, lists, histories="train", by="checkin"):
        assert by == "checkin" and tuple(lists.shape) == (len(se), 2)
        per = {0: [[1.0, 1.0], [-2.0, 0.0], [3.0, float("nan")]], 1: [[0.5, 0.5]], 2: [], 3: [[0.0, 0.0], [0.0, 0.0]]}
        rows = [per[int(u)] for u in se]
        off = np.r_[0, np.cumsum([len(r) for r in rows])]
        delta = np.array([d for r in rows for d in r], np.float64).reshape(-1, 2)
        return torch.zeros((len(se), 2), dtype=torch.float64), torch.as_tensor(delta), torch.as_tensor(off), None


def test_attribution_by_recency_on_a_hand_made_model():
    toy = _Toy()
    out = E.attribution_by_recency(toy, [np.arange(0, 2), np.arange(2, 4)], 2, explain=toy.explain)
    # user 0: |delta| per position 2, 2, 3 (the NaN entry counts nothing) -> shares 2/7, 2/7, 3/7, last first; user 1: 1; user 2 has no history,
    # user 3 no attribution at all (all-zero deltas): neither counts
    assert out["rows"] == 2 and out["share"].tolist() == pytest.approx([(3 / 7 + 1) / 2, 2 / 7, 2 / 7]) and out["count"].tolist() == [2, 1, 1]
