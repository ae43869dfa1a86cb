"""CPU tests of the restricted recommendation's host side: the oracle's candidate sets (tests/near_oracle.py) against a brute-force
cal_dis <= r, and the exclusion lists of data.py (sorted, unique; bad lists raise).  No GPU."""
import numpy as np
import pytest

from poi_amd import data as D
from tests import near_oracle as NO


@pytest.fixture(autouse=True)
def _binding_declares_the_entry_point():
    import poi_amd
    assert "poi_score_topk_near" in poi_amd._lib.SIGNATURES, "the oracle checks below stand for a kernel the library must export"


def _coords(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack((30.0 + rng.uniform(0, 40.0 / 111.0, n), 120.0 + rng.uniform(0, 40.0 / 96.0, n)), axis=1)


@pytest.mark.parametrize("r_km", [0.0, 2.0, 8.0, 25.0, 1000.0])
def test_oracle_candidate_sets_equal_brute_force(r_km):
    xy = _coords(1, 200)
    xy[17] = xy[5]; xy[140] = xy[5]                      # co-located POIs: inside every radius, 0 included
    anchor = np.array([5, 0, 199, 63, 17])
    m = NO.candidate_mask(xy, anchor, r_km)
    assert np.array_equal(m, NO.brute_force_mask(xy, anchor, r_km))
    assert m[0, [5, 17, 140]].all() and m[np.arange(5), anchor].all()
    if r_km == 0.0:
        assert m[0].sum() == 3 and m[1].sum() == 1
    if r_km == 1000.0:
        assert m.all()
    # the neighbour sets of the FPMC-LR checker, plus the anchor itself
    off, ids = D.fpmc_neighbors_host(xy, r_km)
    for r, a in enumerate(anchor):
        assert np.array_equal(np.nonzero(m[r])[0], np.sort(np.r_[ids[off[a]:off[a + 1]], a]))


def test_no_anchor_and_no_radius_keep_every_poi():
    xy = _coords(2, 200)
    assert NO.candidate_mask(xy, np.array([-1, 3]), 1.0)[0].all()
    assert NO.candidate_mask(xy, np.array([4, 3]), None).all()
    m = NO.candidate_mask(xy, np.array([-1, 3]), None, np.array([0, 2, 3]), np.array([7, 9, 3]))
    assert not m[0, [7, 9]].any() and m[0].sum() == 198 and not m[1, 3] and m[1].sum() == 199


def test_train_and_last_exclusion_lists_are_sorted_and_unique():
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 30, 40)
    off = np.r_[0, np.cumsum(lens)]
    p = rng.integers(0, 201, off[-1])                     # few POIs: repeats; 200 = the padding id
    eo, ids = D.train_exclusion_csr(off, p, 200)
    assert eo[0] == 0 and eo[-1] == len(ids) and ids.dtype == np.int32
    for u in range(40):
        row = ids[eo[u]:eo[u + 1]]
        assert np.array_equal(row, np.unique(p[off[u]:off[u + 1]][p[off[u]:off[u + 1]] < 200]))
    D.check_exclusion_csr(eo, ids, 40, 200)                # ... and pass the check the host lists get
    lo, li = D.last_exclusion_csr([4, -1, 199, 4])
    assert np.array_equal(lo, [0, 1, 1, 2, 3]) and np.array_equal(li, [4, 199, 4])
    D.check_exclusion_csr(lo, li, 4, 200)


def test_bad_exclusion_lists_raise():
    ok_off, ok_ids = [0, 2, 2, 5], [3, 9, 0, 4, 199]
    off, ids = D.check_exclusion_csr(ok_off, ok_ids, 3, 200)
    assert off.dtype == np.int32 and ids.dtype == np.int32 and np.array_equal(ids, ok_ids)
    with pytest.raises(ValueError, match="ascending"):
        D.check_exclusion_csr(ok_off, [9, 3, 0, 4, 199], 3, 200)       # unsorted row
    with pytest.raises(ValueError, match="ascending"):
        D.check_exclusion_csr(ok_off, [3, 3, 0, 4, 199], 3, 200)       # a repeated id
    with pytest.raises(IndexError):
        D.check_exclusion_csr(ok_off, [3, 9, 0, 4, 200], 3, 200)
    with pytest.raises(IndexError):
        D.check_exclusion_csr(ok_off, [-1, 9, 0, 4, 199], 3, 200)
    for bad_off in ([0, 2, 5], [1, 2, 2, 5], [0, 3, 2, 5], [0, 2, 2, 4]):
        with pytest.raises(ValueError, match="offsets"):
            D.check_exclusion_csr(bad_off, ok_ids, 3, 200)


def test_oracle_topk_order_and_fill():
    sc = np.array([[1.0, 3.0, 3.0, 2.0, 5.0]])
    mask = np.array([[True, True, True, True, False]])
    ids, val, cnt = NO.topk(sc, mask, 6)
    assert ids.tolist() == [[1, 2, 3, 0, -1, -1]] and cnt.tolist() == [4] and np.isneginf(val[0, 4:]).all()
    assert not NO.qualifying(sc, mask, 3)[0] and NO.qualifying(sc, np.array([[True, True, False, True, True]]), 3)[0]
