"""CPU tests of the capped recommendation: the oracle of tests/capped_oracle.py by hand and against its own second form, the merge
rule the kernels use (and the shortcut they do not), the fill table and data.grid_labels by hand, evaluate.label_spread, the
declarations, and that the cases of tests/capped_cases.py contain what they claim."""
import os
import re

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D
from poi_amd import evaluate as E
from tests import capped_cases as CC
from tests import capped_oracle as CO
from tests import filter_cases as FC
from tests import filter_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc")


def random_problem(rng, n_item=None, ties=None):
    n_item = int(rng.integers(5, 200)) if n_item is None else n_item
    ties = bool(rng.integers(0, 2)) if ties is None else ties
    sc = (rng.integers(0, 6, n_item) if ties else rng.normal(size=n_item)).astype(np.float32)
    lab = rng.integers(0, int(rng.integers(1, 12)), n_item).astype(np.int32)
    lab[rng.random(n_item) < rng.choice([0.0, 0.2])] = -1
    return sc, lab, int(rng.integers(1, 33)), int(rng.integers(1, 5))


# ---- 1: the oracle ------------------------------------------------------------------------------------------------------------------------
def test_the_hand_problem():
    mask = np.ones((1, 12), bool)
    for per, want in CC.HAND_WANT.items():
        for k in (1, 3, 4, 7, 12):
            ids, val, lab, cnt = CO.topk(CC.HAND_SCORES, mask, CC.HAND_LABELS, per, k)
            exp = (want + [-1] * k)[:k]
            assert ids[0].tolist() == exp, (per, k, ids[0])
            assert lab[0].tolist() == [CC.HAND_LABELS[j] if j >= 0 else -1 for j in exp]
            assert val[0].tolist() == [CC.HAND_SCORES[0, j] if j >= 0 else -np.inf for j in exp] and cnt[0] == 12
    # an excluded POI gives its place to the next of its label; the unlabelled POI is never capped
    mask[0, 0] = False
    assert CO.topk(CC.HAND_SCORES, mask, CC.HAND_LABELS, 1, 4)[0][0].tolist() == [1, 4, 7, 11]
    lab = CC.HAND_LABELS.copy(); lab[lab == 2] = -5
    assert CO.topk(CC.HAND_SCORES, np.ones((1, 12), bool), lab, 1, 12)[0][0].tolist() == [0, 4, 7, 11, 8, 9, 10, -1, -1, -1, -1, -1]


def test_greedy_equals_counting_and_shorter_lists_are_prefixes():
    rng = np.random.default_rng(11)
    for _ in range(300):
        sc, lab, k, per = random_problem(rng)
        mask = (rng.random((1, len(sc))) < 0.8)
        a = CO.topk(sc[None], mask, lab, per, k)
        b = CO.topk(sc[None], mask, lab, per, k, form=CO.counting)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        k2 = int(rng.integers(1, k + 1))
        c = CO.topk(sc[None], mask, lab, per, k2)
        assert np.array_equal(c[0], a[0][:, :k2]) and np.array_equal(c[1], a[1][:, :k2]) and np.array_equal(c[2], a[2][:, :k2])


def test_no_effective_cap_is_the_filter_oracle():
    rng = np.random.default_rng(12)
    for shape in FC.SCORE_SHAPES:
        F = FC.score_fixture(shape)
        want = FC.score_expected(shape)
        mask, _ = FO.candidate_masks(F["pmask"], F["pred"], len(F["sc"]), *F["ex"])
        N = F["sc"].shape[1]
        for lab, per in ((CC.labeling("zipf", N)[0], 32), (CC.labeling("distinct", N)[0], 1), (np.full(N, -3, np.int32), 1)):
            got = CO.topk(F["sc"], mask, lab, per, 32)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[3], want[2])
        one = CO.topk(F["sc"], mask, CC.labeling("one", N)[0], 3, 32)                # one label for every POI: the plain top-per
        assert np.array_equal(one[0][:, :3], want[0][:, :3]) and (one[0][:, 3:] == -1).all()
    del rng


# ---- 2: the merge rule --------------------------------------------------------------------------------------------------------------------
def test_pairwise_merge_with_recapping_is_the_global_list():
    rng = np.random.default_rng(13)
    for _ in range(300):
        sc, lab, k, per = random_problem(rng)
        want = CO.recap([(float(s), j) for j, s in enumerate(sc)], lab, per, k)
        ids = CO.topk(sc[None], np.ones((1, len(sc)), bool), lab, per, k)[0][0]
        assert [j for _, j in want] == ids[ids >= 0].tolist()                        # recap over everything is the definition
        for strided in (False, True):
            slices = CC.cuts(len(sc), int(rng.integers(1, 9)), strided)
            lists = CC.slice_lists(sc, lab, slices, per, k)
            assert CO.merge_pairwise(lists, lab, per, k) == want


def test_the_shortcut_is_wrong_on_the_planted_problem():
    """Why block_lists_fold / fold_slice_lists are not reused: the plain best 2 k of the union of the slices' lists, capped once."""
    sc, lab, slices, per, k = CC.planted_shortcut_problem()
    lists = CC.slice_lists(sc, lab, slices, per, k)
    assert all(len(l) == 2 for l in lists)
    want = [(100.0, 0), (14.0, 9)]
    assert CO.recap([(float(s), j) for j, s in enumerate(sc)], lab, per, k) == want
    assert CO.merge_pairwise(lists, lab, per, k) == want
    assert CO.merge_best_then_cap(lists, lab, per, k) == [(100.0, 0)]               # one strong label crowds the others out
    assert CO.merge_best_then_cap(lists, lab, per, k, depth=64) == want             # (deep enough for THIS problem only)


def test_the_adversarial_merge_case_defeats_the_shortcut_at_every_grid():
    users, items, sc = CC.merge_tables()
    lab = CC.merge_labels()
    N, ntile = sc.shape[1], (sc.shape[1] + 31) // 32
    assert np.array_equal((users @ items.T).astype(np.float32), sc)                  # exact products
    for i, S in enumerate(CC.GRIDS):
        slices = [np.arange(32 * (ntile * s // S), min(32 * (ntile * (s + 1) // S), N)) for s in range(S)]
        lists = CC.slice_lists(sc[i], lab, slices, 1, 32)
        want = CO.recap([(float(v), j) for j, v in enumerate(sc[i])], lab, 1, 32)
        assert [lab[j] for _, j in want] == list(range(32)) and [v for v, _ in want] == [100000.0 - 1000 * L for L in range(32)]
        for L in range(32):                                                          # label L's best POI lies in slice L % S
            assert want[L][1] in slices[L % S]
        assert CO.merge_pairwise(lists, lab, 1, 32) == want
        if S > 2:
            assert CO.merge_best_then_cap(lists, lab, 1, 32, depth=64) != want


# ---- 3: fill ------------------------------------------------------------------------------------------------------------------------------
def test_fill_by_hand():
    #            0  1  2  3  4  5   6  7  8  9
    lab = np.array([0, 0, 0, 1, 1, -1, 2, 7, -4, 0])                               # n_label 3: label 7 is a stray
    pm = np.array([[1] * 10, [1, 1, 0, 1, 0, 0, 1, 1, 1, 0], [0] * 10], bool)
    fill, counts, strays = CO.fill_table(lab, 3, pm)
    assert strays == 1 and counts.tolist() == [4, 2, 1]
    # predicate 0: unlabelled 5, 8 and the stray 7 = 3; labels hold 4, 2, 1 POIs
    assert fill[0, :6].tolist() == [3, 6, 8, 9, 10, 10] and fill[0, 32] == 10
    # predicate 1 passes 0, 1 (label 0), 3 (label 1), 6 (label 2), 7 (stray), 8 (unlabelled)
    assert fill[1, :4].tolist() == [2, 5, 6, 6] and (fill[2] == 0).all()
    one, _, _ = CO.fill_table(lab, 3)
    assert np.array_equal(one, fill[:1])
    # fill[q][per] is the length of the longest capped list: the oracle's list on all-equal scores
    for q in range(3):
        for per in (1, 2, 3):
            ids = CO.topk(np.zeros((1, 10), np.float32), pm[q:q + 1], np.where(lab >= 3, -1, lab), per, 10)[0][0]
            assert (ids >= 0).sum() == fill[q, per]


# ---- 4: data.grid_labels ------------------------------------------------------------------------------------------------------------------
def test_grid_labels_by_hand():
    km_per_deg = 12742 * np.pi / 360
    # at the equator (mean latitude ~0) a 1 km cell is 1 / km_per_deg degrees both ways
    d = 1.0 / km_per_deg
    xy = np.array([[0.5 * d, 2.5 * d], [0.6 * d, 2.1 * d],                         # two POIs in one cell
                   [0.5 * d, -0.5 * d], [0.5 * d, 0.5 * d],                        # either side of the 0 degree meridian: two cells
                   [-0.4 * d, 0.2 * d],                                            # south of the equator: another cell
                   [0.9 * d, 0.9 * d],                                             # with POI 3
                   [0.2 * d, 2.9 * d]])                                            # with POIs 0 and 1
    lab, n_label, centres = D.grid_labels(xy, 1.0)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 0, 1, 2, 3, 2, 0] and n_label == 4      # numbered by first appearance
    assert centres.shape == (4, 2)
    step = np.array([d, d / np.cos(xy[:, 0].mean() * np.pi / 180)])
    assert np.allclose(centres / step, [[0.5, 2.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]], atol=1e-6)
    # the longitude step grows with 1 / cos(mean latitude): at 60 degrees two POIs 1.5 km of longitude apart share a 1 km cell
    # column only if the step were not scaled
    lat = 60.0
    dlon_km = km_per_deg * np.cos(lat * np.pi / 180)                               # km per degree of longitude there
    xy = np.array([[lat, 10.0], [lat, 10.0 + 0.9 / dlon_km], [lat, 10.0 + 5.0 / dlon_km]])
    lab, n_label, _ = D.grid_labels(xy, 1.0)
    assert n_label >= 2 and lab[0] != lab[2]
    cells = np.floor(xy[:, 1] / (d / np.cos(lat * np.pi / 180)))
    assert (lab[0] == lab[1]) == (cells[0] == cells[1])
    big = D.grid_labels(np.random.default_rng(3).uniform([40, -75], [41, -73], (5000, 2)), 1.0)
    assert big[1] > 1000 and big[0].max() == big[1] - 1 and np.array_equal(np.unique(big[0]), np.arange(big[1]))
    first = np.array([np.nonzero(big[0] == c)[0][0] for c in range(big[1])])
    assert np.all(np.diff(first) > 0)
    with pytest.raises(ValueError):
        D.grid_labels(xy, 0.0)


# ---- 5: label_spread, declarations -------------------------------------------------------------------------------------------------------
def test_label_spread():
    lab = np.array([0, 0, 1, 2, -1, -1])
    idx = np.array([[0, 1, 2, -1], [0, 2, 3, 4], [-1, -1, -1, -1], [4, 5, -1, -1]])
    distinct, share = E.label_spread(idx, lab)
    assert distinct.tolist() == [2, 4, 0, 2]
    assert np.allclose(share[[0, 1, 3]], [2 / 3, 1 / 4, 1 / 2]) and np.isnan(share[2])


def test_header_and_binding_declare_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "/* additive to 9: capped recommendation - new entry points poi_labels_build, poi_score_topk_capped and poi_topk_capped_scores" in flat
    assert "#define POI_ABI_VERSION 9" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("poi_labels_build", 10), ("poi_score_topk_capped", 29), ("poi_topk_capped_scores", 20)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == n_args, name
        assert name in poi_amd._lib.SIGNATURES and len(poi_amd._lib.SIGNATURES[name][1]) == n_args, name
    for key in ("capped_splits", "capped_split_max"):
        assert key in poi_amd._lib.PLAN_KEYS
    src = open(os.path.join(CSRC, "abi.hip")).read()
    for opt in ("capped_split_max", "capped_grid", "capped_hist_kb"):
        assert '"%s"' % opt in src, opt
    assert "capped.hip" in poi_amd.build.SOURCES
    for fn in ("compute_sub_topk_capped", "poi_labels"):
        assert callable(getattr(poi_amd.models._Base, fn))
    assert callable(poi_amd.models.PoiLabels.from_categories)


# ---- 6: the cases contain what they claim -------------------------------------------------------------------------------------------------
def test_the_labelings_are_what_they_say():
    for N in (1003, 4099):
        sizes = {name: CC.labeling(name, N) for name in CC.LABELINGS}
        assert sizes["one"][1] == 1 and sizes["distinct"][1] == N and sizes["three"][1] == 3 and sizes["by id"][1] == 8
        assert sizes["zipf"][1] == 36 and (sizes["zipf"][0] == 35).sum() == 3
        mixed = sizes["mixed"][0]
        assert (mixed < 0).sum() == len(range(3, N, 7)) and len(np.unique(mixed[mixed < 0])) == 5
        assert np.all(np.diff(sizes["by id"][0]) >= 0)
        for lab, n_label in sizes.values():
            assert lab.dtype == np.int32 and lab.max() < n_label <= N


def test_the_tie_tables_tie_where_they_should():
    users, items, sc = CC.tie_tables()
    assert np.array_equal((users @ items.T).astype(np.float32), sc)
    lab = CC.labeling("zipf", sc.shape[1])[0]
    mask = np.ones(sc.shape, bool)
    for per in (1, 2):
        ids, val, _, _ = CO.topk(sc, mask, lab, per, 20)
        for r in range(len(sc)):
            order, s = CO.ranked(sc[r], mask[r])
            last = val[r][ids[r] >= 0][-1]
            assert (s == last).sum() > 1                                             # the last place is inside a tie
    assert np.signbit(sc[28:][sc[28:] == 0]).any() and not np.signbit(sc[28:][sc[28:] == 0]).all()


def test_the_oracle_alone_leaves_the_independence_rows_qualifying():
    """The seeds of CC.ORACLE_SEEDS: at least 90 % of the rows have clear gaps down to the depth the cap looks at, per 1 and 2."""
    for kind, dim in CC.ORACLE_SEEDS:
        F, osc, mask, lab = CC.oracle_case(kind, dim)
        for per in CC.ORACLE_PERS:
            ok, depth = CO.qualifying(osc, mask, lab, per, FC.K)
            print("%s dim %d per %d: %.0f %% qualify, depth up to %d" % (kind, dim, per, 100 * ok.mean(), depth.max()))
            assert ok.mean() >= 0.9, (kind, dim, per, ok.mean())
