"""The planted top-K fixtures (tests/topk_streams.py) are what they claim to be - checked without a GPU, and without reading kernel
state: exact in float32, long candidate lists from any range partition, and a plateau that really spans item ranges."""
import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import topk_streams as TS

KS = (1, 2, 5, 10, 20, 31, 32)


@pytest.mark.parametrize("N", [1, 33, 65, 129, 2065, 8209])
def test_every_builder_is_float32_exact(N):
    for K in (1, 5, 32, 64):
        names, S = TS.family_rows(N, K, with_g=True)
        for name, row in zip(names, S):
            assert TS.is_exact(row), (name, N, K)
            assert np.array_equal(row.astype(np.float32).astype(np.float64), row), (name, N, K)
        names, S = TS.filter_rows(N, K)
        assert TS.is_exact(S) and np.abs(S).max() <= 65.0, (N, K)
    users, items, full = TS.one_hot(TS.filter_rows(N, 5)[1], 70, 64, n_cls=11)
    assert np.array_equal(users.astype(np.float64) @ items.astype(np.float64).T, full[np.arange(70) % 11])
    users, items, full = TS.one_hot(TS.family_rows(N, 5, with_g=True)[1], 70, 64)
    assert np.array_equal(users.astype(np.float64) @ items.astype(np.float64).T, full[np.arange(70) % 64])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("builder", [TS.staircase_up, TS.staircase_up_mirrored])
def test_rising_staircases_reach_the_long_lists_from_any_range(builder, K):
    """The second readlane loop and the upper-half K-th best of compact_user need a list of 65 .. 80 entries at a compaction; K = 32
    fills slot 79.  From every range start tile (the pattern has period 4: 0 .. 11 covers every phase three times) and every range
    length >= 8 tiles.  Scratch run of the model: 65 / 66 / 69 / 74 / 68 / 79 / 80 for K = 1 / 2 / 5 / 10 / 20 / 31 / 32."""
    row = builder(2065 + 32 * 12)
    for t0 in range(12):
        for nt in (8, 9, 10, 11, 12):
            lens, lst = TS.list_model(row, K, t0, nt)
            assert max(lens) >= 65, (t0, nt, lens)
            if K == 32:
                assert max(lens) == 80, (t0, nt, lens)
            seg = row[None, 32 * t0:32 * (t0 + nt)]
            assert [j for _, j in lst] == list(O.topk_desc(seg, K)[0] + 32 * t0)      # (the model itself selects what the oracle selects)


@pytest.mark.parametrize("K", KS)
def test_falling_staircase_compacts_once_at_64(K):
    """No falling row can hold more than 64 entries at a compaction: the first one comes after two tiles (everything beats -inf) and
    leaves the K-th best of the two HIGHEST tiles of the range as threshold - nothing later passes.  That is the other extreme the
    kernels must get right (one compaction, then only rejections), and the reason family a has a mirrored twin that rises."""
    row = TS.staircase_down(2065 + 32 * 12)
    for t0 in range(12):
        for nt in (8, 9, 11):
            lens, lst = TS.list_model(row, K, t0, nt)
            assert lens == [64], (t0, nt, lens)
            assert max(j for _, j in lst) < 32 * (t0 + 2)                             # all from the first two tiles
            assert [j for _, j in lst] == list(O.topk_desc(row[None, 32 * t0:32 * (t0 + nt)], K)[0] + 32 * t0)


@pytest.mark.parametrize("K", (5, 20, 31, 32))
@pytest.mark.parametrize("value", (2.5, 0.0))
def test_plateau_spans_item_ranges_at_the_cut(K, value):
    N = 2065
    row = TS.plateau(N, K, value)
    exp = O.topk_desc(row[None], K)[0]
    cut = row[exp[-1]]
    assert cut == value and int((row > cut).sum()) == K - 3 and int((row == cut).sum()) >= 200
    members = np.flatnonzero(row == cut)
    assert list(exp[-3:]) == list(members[:3])                 # the lowest-index plateau members close the list
    per_range = [int(((members >= q * (N // 4)) & (members < (q + 1) * (N // 4))).sum()) for q in range(4)]
    assert sum(c > K for c in per_range) >= 2, per_range
    late = TS.plateau_late(N, K, value)
    m2 = np.flatnonzero(late == value)
    assert list(m2[:3]) == [250, 260, 270] and int((late > value).sum()) == K - 3 and list(O.topk_desc(late[None], K)[0][-3:]) == [250, 260, 270]


def test_expected_lists_contract():
    S = np.array([[1.0, np.nan, -np.inf, 1.0, 0.5], [np.nan, -np.inf, -np.inf, np.nan, -np.inf]])
    idx, sc = TS.expected_lists(S, 4, O.topk_desc)
    assert idx.tolist() == [[0, 3, 4, -1], [-1, -1, -1, -1]]
    assert sc[0].tolist() == [1.0, 1.0, 0.5, -np.inf] and np.all(np.isneginf(sc[1]))


@pytest.mark.parametrize("K", (1, 5, 20, 31, 32))
@pytest.mark.parametrize("N", (2065, 8209))
def test_filter_rows_cannot_overflow_the_survivor_lists(N, K):
    """4096 survivor slots per user: within 0.5 of its K-th best score (several times the f16 bound at these magnitudes) every filter
    row keeps fewer items than that; sparse g holds sixteen float32 values that are two values in half precision."""
    names, S = TS.filter_rows(N, K)
    for name, row in zip(names, S):
        kth = np.sort(row)[::-1][K - 1]
        assert int((row > kth - 0.5).sum()) < 4096, (name, int((row > kth - 0.5).sum()))
    g = S[names.index("g sparse half planes")]
    m = g[g >= 64.0]
    assert len(np.unique(m)) == 16 and len(np.unique(m.astype(np.float16))) == 2 and len(m) > 2 * 32
