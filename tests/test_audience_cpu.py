"""CPU tests of the audience recommendation's host side: the oracle against a brute force, data.visitors_csr against sets and as the
inverse of data.train_exclusion_csr, the host argument checks of models.recommend_audience, the launch planner (csrc/audience_plan.h)
compiled on its own at its boundaries, and the condition on the fixtures of tests/test_gpu_audience.py - at least 90 % of the queries of
every fixture have clear top-(k + 1) gaps under the oracle alone (the rule and the bar of tests/test_group_cpu.py), so that a float32
kernel must rank them exactly.  No GPU."""
import shutil
import subprocess

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D, models as M
from tests import audience_cases as AC
from tests import audience_oracle as AO


def test_oracle_matches_a_brute_force():
    rng = np.random.default_rng(1)
    users, items = rng.uniform(-1, 1, (9, 3)), rng.uniform(-1, 1, (7, 3))        # (items: 6 POIs + the padding row)
    pois = [4, 0, 4, 5]
    ex = [[1, 7], [], list(range(9)), [0, 2, 3, 4, 5, 8]]
    eo, ei = AO.csr(ex)
    sct = AO.scores_t(users, items)
    assert sct.shape == (6, 9) and np.allclose(sct, (users @ items[:-1].T).T, rtol=1e-14, atol=0)
    got = AO.topk(sct[pois], AO.candidate_mask(len(pois), 9, eo, ei), 4)
    want, cnt = AO.brute_force(users, items, pois, 4, [set(e) for e in ex])
    assert np.array_equal(got[0], want) and np.array_equal(got[2], cnt) and cnt.tolist() == [7, 9, 0, 3]
    assert np.all(got[0][2] == -1) and np.all(np.isneginf(got[1][2])) and got[0][3].tolist()[3] == -1
    free = AO.topk(sct[pois], AO.candidate_mask(len(pois), 9), 9)
    assert np.array_equal(free[0], AO.brute_force(users, items, pois, 9)[0]) and np.array_equal(free[0][0], free[0][2])


def test_the_distance_term_follows_the_rows_last_poi():
    """The transposed matrix keeps near_oracle's term: a row without a last POI has none."""
    R = AC.rank_case("spatial", 32)
    C = R["C"]
    plain = AO.scores_t(C["users"], C["items"])
    for r in AC.NO_LAST:
        assert R["last"][r] == -1 and np.array_equal(R["sct"][:, r], plain[:, r])
    others = np.setdiff1d(np.arange(AC.N_USER), AC.NO_LAST)
    assert (R["sct"][:, others] != plain[:, others]).mean() > 0.5


def test_visitors_csr_against_sets_and_as_the_inverse_of_the_train_exclusion():
    rng = np.random.default_rng(2)
    n_user, n_item = 40, 23
    lens = rng.integers(0, 9, n_user)
    off = np.r_[0, np.cumsum(lens)]
    p = rng.integers(0, n_item + 1, off[-1])                                 # (the padding id n_item is no visit)
    vo, vu = D.visitors_csr(off, p, n_item)
    assert vo.dtype == np.int64 and vu.dtype == np.int32 and vo.shape == (n_item + 1,) and vo[0] == 0 and vo[-1] == len(vu)
    sets = AO.visitor_sets([p[a:b] for a, b in zip(off[:-1], off[1:])], n_item)
    for j in range(n_item):
        assert vu[vo[j]:vo[j + 1]].tolist() == sorted(sets[j]), j
    D.check_exclusion_csr(vo, vu, n_item, n_user)                            # ascending and unique within every POI
    eo, ex = D.train_exclusion_csr(off, p, n_item)
    pairs = {(u, int(j)) for u in range(n_user) for j in ex[eo[u]:eo[u + 1]]}
    assert pairs == {(int(u), j) for j in range(n_item) for u in vu[vo[j]:vo[j + 1]]} and len(pairs) == len(vu) == len(ex)
    # the inverse of the inverse: the visitor lists read as a "train table" of POIs give the exclusion lists back
    bo, bx = D.visitors_csr(vo, vu, n_user)
    assert np.array_equal(bo, eo) and np.array_equal(bx, ex)
    vo0, vu0 = D.visitors_csr(np.zeros(1, np.int64), np.zeros(0, np.int64), 5)
    assert vo0.tolist() == [0] * 6 and len(vu0) == 0
    lists = AO.visitor_lists([p[a:b] for a, b in zip(off[:-1], off[1:])], n_item, [3, 3, 0], segment=np.arange(1, n_user, 2))
    for q, j in enumerate([3, 3, 0]):
        assert lists[1][lists[0][q]:lists[0][q + 1]].tolist() == [(u - 1) // 2 for u in sorted(sets[j]) if u % 2]


def test_host_argument_checks():
    seg = M._Base._audience_segment
    assert seg(None, 9) is None and seg([2, 5, 8], 9).tolist() == [2, 5, 8] and seg(np.zeros(0, int), 9).size == 0
    for bad in ([0, 9], [-1, 3]):
        with pytest.raises(IndexError):
            seg(bad, 9)
    for bad in ([5, 3], [3, 3], [0, 2, 2, 4]):
        with pytest.raises(ValueError, match="ascending"):
            seg(bad, 9)
    obj = M._Base()
    assert obj._audience_k(32, 6, True) == 32 and obj._audience_k(1, 6, True) == 1 and obj._audience_k(33, 100, True) == 33
    assert obj._audience_k(4096, 5000, True) == 4096 and obj._audience_k(6, 6, False) == 6
    for k, n, fused in ((0, 100, True), (33, 32, True), (4097, 5000, True), (101, 100, True), (7, 6, False), (0, 6, False)):
        with pytest.raises(ValueError, match="audience"):
            obj._audience_k(k, n, fused)


_MAIN = r"""
#include <stdio.h>
#include "audience_plan.h"
int main() {
  int n_q, n, split_max, grid_opt, num_cu;
  while (scanf("%d %d %d %d %d", &n_q, &n, &split_max, &grid_opt, &num_cu) == 5) {
    const SplitPlan P = audience_plan(n_q, n, split_max, grid_opt, num_cu);
    printf("%d %d\n", P.split, P.n_split);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("audience_plan")
    cxx = shutil.which("c++") or shutil.which("g++") or poi_amd.build._hipcc()
    src, exe = str(d / "audience_plan_main.cpp"), str(d / "audience_plan_main")
    open(src, "w").write(_MAIN)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", poi_amd.build.CSRC, src, "-o", exe], check=True)      # alone: no HIP anywhere near it

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        got = [tuple(int(v) for v in line.split()) for line in out if line]
        assert len(got) == len(cases)
        return got
    return run


def _plan(n_q, n, split_max, grid_opt, num_cu):
    """The rule, re-spelled: at most split_max queries take the slices; the grid option as given, otherwise two workgroups per CU over
    the query blocks while a slice keeps 16 user tiles; at least one slice, at most 64."""
    if n_q > split_max:
        return (0, 1)
    s = grid_opt
    if grid_opt <= 0:
        s = max(1, min(2 * num_cu // max((n_q + 31) // 32, 1), ((n + 31) // 32) // 16))
    return (1, min(s, 64))


def test_the_plan_header_at_its_boundaries(planner):
    cases = [(n_q, n, split_max, grid, cu) for n_q in (1, 31, 32, 33, 256, 257, 1024, 100000) for n in (0, 1, 511, 512, 513, 1037, 32768, 50000, 10 ** 7)
             for split_max in (0, 1, 256, 1 << 30) for grid in (0, 1, 7, 64) for cu in (1, 256, 304)]
    got = planner(cases)
    for c, g in zip(cases, got):
        assert g == _plan(*c), (c, g)
    named = {c: g for c, g in zip(cases, got)}
    assert named[(1, 50000, 256, 0, 256)] == (1, 64)          # one POI against 50 k users: the cap of the merge
    assert named[(256, 50000, 256, 0, 256)] == (1, 64) and named[(257, 50000, 256, 0, 256)] == (0, 1)      # the switch point
    assert named[(1, 1037, 256, 0, 256)] == (1, 2)            # 33 user tiles: two slices of 16 and 17
    assert named[(1, 511, 256, 0, 256)] == (1, 1) and named[(1, 0, 256, 0, 256)] == (1, 1)      # the floor
    assert named[(100000, 50000, 1 << 30, 0, 256)] == (1, 1)  # more query blocks than CU slots
    assert named[(33, 1037, 1 << 30, 64, 256)] == (1, 64) and named[(33, 1037, 0, 64, 256)] == (0, 1)


def test_fixtures_have_clear_gaps():
    for name, sc, mask in AC.fixtures():
        ok = AO.qualifying(sc, mask, AC.K)
        print("%s: %.1f %% of %d queries qualify, candidates %d..%d" % (name, 100 * ok.mean(), len(ok), mask.sum(axis=1).min(), mask.sum(axis=1).max()))
        assert sc.shape == (AC.N_QUERY, AC.N_USER) and mask.sum(axis=1).max() < AC.N_USER, name
        assert ok.mean() >= 0.9, "%s: only %.1f %% of the queries have clear gaps: pick another seed" % (name, 100 * ok.mean())


def test_the_half_rounding_moves_the_oracle_beyond_the_margin():
    """A kernel that served the float32 init could not pass the half cases: the rounding moves the scores by more than RTOL max|score|."""
    from tests.gpu_util import RTOL
    for kind, dim in AC.HALF_CASES:
        R = AC.half_case(kind, dim)
        assert np.abs(R["sct"] - R["sct32"]).max() > 4 * RTOL * np.abs(R["sct"]).max(), (kind, dim)
