"""CPU tests of the label recommendation: the oracle of tests/labels_oracle.py by hand, its additivity, its by-max order against the
capped oracle at per = 1, a planted problem on which the mass and the max order differ, the declarations, and that the cases of
tests/labels_cases.py contain what they claim - above all that the float64 oracle ALONE leaves at least 90 % of their rows clear."""
import os
import re

import numpy as np
import pytest

import poi_amd
from tests import capped_oracle as CO
from tests import labels_cases as LC
from tests import labels_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc")
U = 1 << LO.Q_BITS
LOG_ATOL = 2e-14      # log p is the difference of two float64 logs near 36 log 2 = 25: half an ulp (1.8e-15) each from the log, one from the subtraction


# ---- 1: the oracle ------------------------------------------------------------------------------------------------------------------------
def test_the_hand_problem():
    D = LO.dense(LC.HAND_SCORES, None, LC.HAND_LABELS, LC.HAND_N_LABEL)
    assert D["M"][0] == 0.0
    assert D["mass"].dtype == np.uint64 and [int(x) for x in D["mass"][0]] == [q * (U // 4) for q in LC.HAND_MASS_QUARTERS]
    assert D["best_id"][0].tolist() == LC.HAND_BEST and D["count"][0].tolist() == LC.HAND_COUNT
    assert int(D["total"][0]) == 23 * (U // 4)
    assert np.isneginf(D["best_score"][0, 3]) and D["best_score"][0, 2] == -LC.LN2
    for by, order in LC.HAND_ORDER.items():
        for k in (1, 2, 3, 4, 32):
            T = LO.topk(D, by, k)
            want = (order + [-1] * k)[:k]
            assert T["label"][0].tolist() == want and T["n_listed"][0] == min(k, 3), (by, k)
            assert T["best_id"][0].tolist() == [LC.HAND_BEST[l] if l >= 0 else -1 for l in want]
            lp = [np.log(LC.HAND_MASS_QUARTERS[l] / 23.0) if l >= 0 else -np.inf for l in want]
            assert np.allclose(T["logp"][0], lp, rtol=0, atol=LOG_ATOL), (by, k)
            assert np.isclose(T["rest_logp"][0], np.log(1 / 23.0), rtol=0, atol=LOG_ATOL)
    assert np.isclose(LO.lognorm(D)[0], np.log(23 / 4.0), rtol=0, atol=LOG_ATOL)
    # without POI 0: A = 5/4 u ties B in mass - the lower label first - and A's best is POI 1; M is still 0
    mask = np.ones((1, 12), bool); mask[0, 0] = False
    E = LO.dense(LC.HAND_SCORES, mask, LC.HAND_LABELS, LC.HAND_N_LABEL)
    assert E["M"][0] == 0.0 and int(E["mass"][0, 0]) == int(E["mass"][0, 1]) == 5 * (U // 4) and E["best_id"][0, 0] == 1
    assert LO.topk(E, "mass", 3)["label"][0].tolist() == [2, 0, 1] and LO.topk(E, "max", 3)["label"][0].tolist() == [1, 0, 2]
    assert int(D["mass"][0, 0]) - int(E["mass"][0, 0]) == U          # exactly the excluded POI's term


def test_rows_without_a_finite_maximum_are_fill():
    sc = np.array([[np.nan, np.nan, np.nan], [1.0, np.inf, 0.0], [-np.inf, -np.inf, np.nan], [np.nan, -2.0, -np.inf]])
    D = LO.dense(sc, None, [0, 1, 1], 2)
    assert np.isneginf(D["M"][0]) and np.isposinf(D["M"][1]) and np.isneginf(D["M"][2]) and D["M"][3] == -2.0
    assert not D["count"][:3].any() and not D["mass"][:3].any() and (D["best_id"][:3] == -1).all()
    assert D["count"][3].tolist() == [0, 1, 0] and int(D["mass"][3, 1]) == U      # a NaN and a -inf score are no candidates
    T = LO.topk(D, "mass", 2)
    assert (T["label"][:3] == -1).all() and np.isneginf(T["logp"][:3]).all() and T["label"][3].tolist() == [1, -1]
    assert np.isneginf(LO.lognorm(D)[:3]).all() and LO.lognorm(D)[3] == -2.0


def test_zeros_of_both_signs_are_one_score():
    D = LO.dense(np.array([[-0.0, 0.0, -1.0]], np.float32), None, [0, 0, 0], 1)
    assert D["best_id"][0, 0] == 0 and not np.signbit(D["best_score"][0, 0]) and not np.signbit(D["M"][0])


def test_mass_is_additive_over_partitions_of_the_candidates():
    rng = np.random.default_rng(31)
    for _ in range(40):
        N, L = int(rng.integers(5, 300)), int(rng.integers(1, 9))
        sc = rng.normal(size=(3, N)).astype(np.float32) * rng.choice([0.3, 3.0, 10.0])
        lab = rng.integers(-1, L, N)
        full = LO.dense(sc, None, lab, L)
        part = rng.integers(0, int(rng.integers(1, 6)), (3, N))
        pieces = [LO.dense(sc, part == s, lab, L) for s in range(int(part.max()) + 1)]
        assert all(np.array_equal(P["M"], full["M"]) for P in pieces)                 # M does not depend on the candidates
        assert np.array_equal(sum(P["mass"] for P in pieces), full["mass"])
        assert np.array_equal(sum(P["count"] for P in pieces), full["count"])
        # the best of the whole is the best of the pieces' bests under better()
        stack = np.stack([LO.f64(P["best_score"]) for P in pieces]), np.stack([P["best_id"] for P in pieces])
        for r in range(3):
            for b in range(L + 1):
                c = [(-(stack[0][s][r, b]), stack[1][s][r, b]) for s in range(len(pieces)) if stack[1][s][r, b] >= 0]
                assert (min(c)[1] if c else -1) == full["best_id"][r, b]
        assert np.array_equal(LO.dense(sc, None, lab, L)["total"], full["mass"].sum(axis=1, dtype=np.uint64))


def test_by_max_is_the_capped_oracle_at_per_one():
    rng = np.random.default_rng(32)
    for _ in range(60):
        N, L = int(rng.integers(5, 300)), int(rng.integers(1, 40))
        ties = bool(rng.integers(0, 2))
        sc = (rng.integers(0, 5, (4, N)) if ties else rng.normal(size=(4, N))).astype(np.float32)
        lab = rng.integers(0, L, N).astype(np.int32)                                  # (no unlabelled POIs: capped lists those too)
        mask = rng.random((4, N)) < 0.8
        for k in (1, 5, 32):
            T = LO.topk(LO.dense(sc, mask, lab, L), "max", k)
            ids, val, labs, _ = CO.topk(sc, mask, lab, 1, k)
            assert np.array_equal(T["label"], labs) and np.array_equal(T["best_id"], ids)
            assert np.array_equal(T["best_score"].view(np.uint32), val.view(np.uint32))


def test_the_planted_problem_orders_differently_by_mass_and_by_max():
    sc, lab = LC.planted_orders()
    D = LO.dense(sc, None, lab, 5)
    by_mass, by_max = LO.topk(D, "mass", 5), LO.topk(D, "max", 5)
    assert by_mass["label"][0].tolist() == [0, 1, 2, 3, 4] and by_max["label"][0].tolist() == [1, 0, 2, 3, 4]
    assert np.isclose(np.exp(by_mass["logp"][0, 0]), 400 * np.e / (400 * np.e + np.exp(3) + np.exp(0.5) + np.exp(-0.5) + np.exp(-1.5)), rtol=1e-9)
    assert LO.clear_rows(D, sc, "mass", 4).all() and LO.clear_rows(D, sc, "max", 4).all()
    assert np.isneginf(by_mass["rest_logp"][0]) and D["count"][0, 5] == 1003 - 404   # the unlabelled POIs at -30 add nothing: exp(-33) 2^36 < 1/2


def test_the_clear_row_rule():
    lab = np.arange(4)
    sc = np.log(np.array([[4.0, 3.0, 2.0, 1.0], [4.0, 4.0 * (1 + 1e-7), 2.0, 1.0], [4.0, 3.0, 2.0, 2.0 * (1 + 1e-7)]]))
    D = LO.dense(sc, None, lab, 4)
    assert LO.clear_rows(D, sc, "mass", 3).tolist() == [True, False, False]             # the pair behind the list (k + 1) counts too
    assert LO.clear_rows(D, sc, "mass", 2).tolist() == [True, False, True]
    assert LO.clear_rows(D, sc, "max", 3).tolist() == [True, False, False]


# ---- 2: the declarations ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "/* additive to 9: label recommendation - new entry points poi_score_labels, poi_score_topk_labels and poi_labels_scores" in flat
    assert "#define POI_ABI_VERSION 9" in hdr
    assert "ABSOLUTE ERROR FLOOR of 2^-37 of the best POI's weight" in flat and "n_item < 2^27" in flat
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("poi_score_labels", 25), ("poi_score_topk_labels", 29), ("poi_labels_scores", 24)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == n_args, name
        assert name in poi_amd._lib.SIGNATURES and len(poi_amd._lib.SIGNATURES[name][1]) == n_args, name
    for key in ("labels_splits", "labels_split_max", "labels_home", "labels_chunks", "labels_rows_per_chunk"):
        assert key in poi_amd._lib.PLAN_KEYS
    src = open(os.path.join(CSRC, "abi.hip")).read()
    for opt in ("labels_split_max", "labels_grid", "labels_lds_kb", "labels_ws_kb"):
        assert '"%s"' % opt in src and '"%s"' % opt in flat, opt
    assert "labels.hip" in poi_amd.build.SOURCES
    for cls in (poi_amd.models._Base, poi_amd.models.Session, poi_amd.models.CellSession):
        assert callable(getattr(cls, "recommend_labels")), cls
    assert callable(poi_amd.models._Base.label_distribution) and callable(poi_amd.evaluate.label_hit_rate)


# ---- 3: the cases -------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_say():
    for name, (n_item, n_label, kind, dim, k, n_dist) in LC.CASES.items():
        C = LC.case(name)
        assert C["users"].shape == (LC.N_ROWS, dim) and C["items"].shape == (n_item + 1, dim) and C["users"].dtype == np.float32
        lab = C["labels"]
        assert lab.dtype == np.int32 and lab.shape == (n_item,) and lab.max() < n_label
        assert (lab < 0).any() == (kind == "mixed")
        off, ids = C["ex"]
        assert off[1] == 0 and off[-1] == len(ids) and (np.diff(off)[1::3] > 0).any()
        for r in range(LC.N_ROWS):
            assert np.all(np.diff(ids[off[r]:off[r + 1]]) > 0)
        assert (C["geo"] is not None) == (n_dist > 0)
        if n_dist:
            g = C["geo"]
            assert g["thr"].shape == (n_dist,) and g["sts"].shape == (LC.N_ROWS, n_dist + 1) and (g["anchor"][[3, 40]] == -1).all()
    assert n_item % 32 and LC.CASES["tiny27"][0] < 32
    empty = [l for l in range(37) if not (LC.case("zipf37")["labels"] == l).any()]
    assert 36 in empty                                                                # a label without a POI
    g = np.bincount(LC.case("grid1681")["labels"], minlength=1681)
    assert (g == 0).any() and g.max() >= 3 and np.median(g[g > 0]) <= 2


def test_the_tie_tables_tie_where_they_should():
    users, items, sc, lab = LC.tie_tables()
    D = LO.dense(sc, None, lab, 7)
    assert np.isnan(sc[:, 5]).all() and np.isneginf(sc[27, 6]) and np.isnan(sc[0, 6])
    assert (D["count"][:, :7].sum(axis=1) + D["count"][:, 7] == 1003 - 2).all()      # the NaN / -inf POIs are no candidates
    assert int(D["mass"][0, 0]) == int(D["mass"][0, 1]) > 0                           # row 0: labels 0 and 1 tie in mass ...
    T = LO.topk(D, "mass", 7)
    at = T["label"][0].tolist()
    assert at.index(0) + 1 == at.index(1)                                             # ... and the lower label comes first
    ties = 0
    for r in range(32):                                                               # best scores tie across labels on every row
        b = D["best_score"][r, :7]
        ties += len(set(b.tolist())) < 7
    assert ties == 32


@pytest.mark.parametrize("name", list(LC.CASES))
def test_the_oracle_alone_leaves_the_rows_clear(name):
    """The cap: at least 90 % of the rows of every fixture the GPU tests use are clear on the float64 oracle alone, in both orders -
    otherwise "exact label lists on the clear rows" would hold too few rows to mean anything."""
    C = LC.case(name)
    osc = LC.oracle_scores(name)
    for mask in (None, LC.ex_mask(C)):
        D = LO.dense(osc, mask, C["labels"], C["n_label"])
        for by in ("mass", "max"):
            ok = LO.clear_rows(D, osc, by, C["k"])
            print("%s by %s: %.1f %% of %d rows clear" % (name, by, 100 * ok.mean(), len(ok)))
            assert ok.mean() >= 0.9, (name, by, ok.mean())
