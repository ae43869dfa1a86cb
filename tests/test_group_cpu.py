"""CPU tests of the group recommendation's host side: the oracle against a brute force, data.group_exclusion_csr against set unions,
the host argument checks of models.recommend_group, and the condition on the fixtures of tests/test_gpu_group.py - at least 90 % of
the groups of every fixture have clear top-(k + 1) gaps under the oracle alone, at both rules (the rule of tests/test_gpu_near.py),
so that a float32 kernel must rank them exactly.  No GPU."""
import numpy as np
import pytest

from poi_amd import data as D, models as M
from tests import group_cases as GC
from tests import group_oracle as GO


def test_oracle_matches_a_brute_force():
    rng = np.random.default_rng(1)
    users, items = rng.uniform(-1, 1, (6, 3)), rng.uniform(-1, 1, (10, 3))       # (items: 9 POIs + the padding row)
    groups = [[0, 1, 2], [4], [], [5, 5, 3]]
    ex = [[1, 7], [], [], [0]]
    off, ids = GO.csr(groups)
    eo, ei = GO.csr(ex)
    sc = GO.member_scores(users, items)
    for agg in GO.AGGS:
        got = GO.topk(GO.aggregate(sc, off, ids, agg), GO.candidate_mask(off, 9, eo, ei), 4)
        for g, mem in enumerate(groups):
            val = {j: (np.mean if agg == "mean" else np.min)([users[m] @ items[j] for m in mem]) for j in range(9) if mem and j not in ex[g]}
            want = sorted(val, key=lambda j: (-val[j], j))[:4]
            assert got[0][g].tolist() == want + [-1] * (4 - len(want)) and got[2][g] == len(val)
            assert np.allclose(got[1][g][:len(want)], [val[j] for j in want], rtol=1e-14, atol=0)


def test_group_exclusion_csr_is_the_union_of_the_members_lists():
    rng = np.random.default_rng(2)
    n_user, n_item = 30, 50
    lens = rng.integers(0, 9, n_user)
    off = np.r_[0, np.cumsum(lens)]
    p = rng.integers(0, n_item + 1, off[-1])                                 # (the padding id n_item is no visit)
    eo, ex = D.train_exclusion_csr(off, p, n_item)
    groups = [[3, 4, 3], [], [7], list(range(n_user)), [29, 0]]
    go, gm = GO.csr(groups)
    xo, xi = D.group_exclusion_csr(eo, ex, go, gm, n_item)
    assert xo.dtype == np.int64 and xi.dtype == np.int32 and xo[0] == 0 and xo[-1] == len(xi)
    for g, mem in enumerate(groups):
        want = sorted({int(v) for m in mem for v in p[off[m]:off[m + 1]] if v < n_item})
        assert xi[xo[g]:xo[g + 1]].tolist() == want, g
    D.check_exclusion_csr(xo, xi, len(groups), n_item)
    with pytest.raises(IndexError):
        D.group_exclusion_csr(eo, ex, [0, 1], [n_user], n_item)
    with pytest.raises(ValueError):
        D.group_exclusion_csr(eo, ex, [0, 2, 1], [1, 2], n_item)


def test_host_argument_checks():
    csr = M._Base._group_csr
    off, ids, dev = csr([[1, 2], [], [3]], 5, "groups")
    assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [1, 2, 3] and not dev
    off, ids, dev = csr((np.array([0, 1, 3]), [4, 0, 0]), 5, "groups")
    assert off.tolist() == [0, 1, 3] and ids.tolist() == [4, 0, 0]
    for bad in ([[1, 5]], [[-1]], ([0, 1], [7])):
        with pytest.raises(IndexError):
            csr(bad, 5, "groups")
    for bad in (([0, 2, 1, 3], [0, 1, 2]), ([1, 3], [0, 1, 2]), ([0, 2], [0, 1, 2]), ([0, 4], [0, 1, 2])):
        with pytest.raises(ValueError):
            csr(bad, 5, "groups")
    uniq, mem = M._Base._group_members(np.array([4, 9, 4, -1, 2]), 5)
    assert uniq.tolist() == [2, 4] and mem.tolist() == [1, -1, 1, -1, 0]
    obj = M._Base()
    assert obj._group_args(32, "min") == (32, 1) and obj._group_args(1, "mean") == (1, 0)
    for k in (0, 33):
        with pytest.raises(M._lib.PoiError, match="k <= 32"):
            obj._group_args(k, "mean")
    with pytest.raises(ValueError):
        obj._group_args(5, "borda")


@pytest.mark.parametrize("agg", GO.AGGS)
def test_fixtures_have_clear_gaps(agg):
    for name, sc, off, ids, eo, ei, k in GC.all_fixtures():
        a = GO.aggregate(sc, off, ids, agg)
        ok = GO.qualifying(a, GO.candidate_mask(off, sc.shape[1], eo, ei), k)
        print("%s %s: %.0f %% of %d groups qualify" % (name, agg, 100 * ok.mean(), len(ok)))
        if name == "ties":
            continue                                     # (planted ties: the fixture of the tie test, not of a ranking test)
        assert ok.mean() >= 0.9, "%s %s: only %.1f %% of the groups have clear gaps: pick another seed" % (name, agg, 100 * ok.mean())
