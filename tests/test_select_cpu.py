"""CPU tests of the candidate generation's host side: the oracle (tests/select_oracle.py) against a brute-force Python sort, the
fixtures of tests/select_cases.py judged under the oracle alone (they contain what they claim), and the declarations of the three
entry points (header, ctypes binding, build list, Python surface).  No GPU."""
import os
import re

import numpy as np

from tests import select_cases as SC
from tests import select_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_against_a_brute_force_sort():
    for shape in ("one", "short", "odd"):
        F = SC.fixture(shape)
        sc = F["sc"][:20]
        n, N = sc.shape
        off, ids = F["ex"]
        for k in (1, 5, 20, 64, 100):
            if k > N:
                continue
            for ex in ((None, None), (off[:n + 1], ids)):
                got = SO.select(sc, k, *ex)
                want = SO.brute_force(sc, k, *ex)
                for r in range(n):
                    m = len(want[r])
                    assert got[0][r, :m].tolist() == want[r] and (got[0][r, m:] == -1).all() and np.isneginf(got[1][r, m:]).all(), (shape, k, r)
                    assert np.array_equal(got[1][r, :m], SO.fold(sc[r])[want[r]])


def test_oracle_rules():
    sc = np.array([[0.0, -0.0, np.nan, -np.inf, np.inf, -0.0, 1.0]], np.float32)
    ids, val, cnt, bad = SO.select(sc, 7)
    assert ids.tolist() == [[4, 6, 0, 1, 5, -1, -1]] and cnt.tolist() == [7] and bad == 0      # the zeros are ONE score: the id decides
    assert not np.signbit(val[0, 2:5]).any() and np.isneginf(val[0, 5:]).all()
    ids, val, cnt, bad = SO.select(sc, 3, np.array([0, 2]), np.array([4, 6]))
    assert ids.tolist() == [[0, 1, 5]] and cnt.tolist() == [5]
    for lst in ([3, 3], [4, 2], [0, 7], [-1, 2]):                                               # not ascending / outside the table
        ids, val, cnt, bad = SO.select(sc, 3, np.array([0, 2]), np.array(lst))
        assert ids.tolist() == [[-1, -1, -1]] and cnt.tolist() == [0] and bad == 1


def _tie_counts(row, ids_row, k):
    """(entries equal to the K-th score inside the list, outside it) of one oracle row."""
    m = int((ids_row[:k] >= 0).sum())
    if m < k:
        return 0, 0
    s = SO.fold(row)
    t = s[ids_row[k - 1]]
    inside = int((s[ids_row[:k]] == t).sum())
    return inside, int((s == t).sum()) - inside


def test_fixtures_contain_what_they_claim():
    seen = set()
    for shape, (n, N) in SC.SHAPES.items():
        F = SC.fixture(shape)
        sc = F["sc"]
        assert sc.shape == (n, N) and sc.dtype == np.float32
        full = SC.expected(shape, False)
        for r in range(n):
            pat, row = SC.pattern_of(r), sc[r]
            seen.add(pat)
            if pat == "plateau":                         # the lowest ids, in order
                assert len(np.unique(row)) == 1 and full[0][r].tolist() == list(range(full[0].shape[1]))
            if pat in ("eight", "eight_signed"):
                assert len(np.unique(SO.fold(row))) <= 8
            if pat == "dead":
                assert (full[0][r] == -1).all() and full[2][r] == N
            if pat == "sparse":
                assert (full[0][r] >= 0).sum() == min(7, N)
            if pat == "ascending":
                assert full[0][r, 0] == N - 1
            if pat == "descending":
                assert full[0][r, 0] == 0
        # the K-th boundary falls INSIDE a tie group, with two or more entries equal to the K-th score on both sides of the cut
        for k in SC.ks_of(N):
            if k < 20 or k >= N // 2:                    # (k = 1 has one entry inside; beyond N / 2 an 8-value row may be cut between groups)
                continue
            for pat in SC.TIE_PATTERNS:
                rows = [r for r in range(n) if SC.pattern_of(r) == pat]
                if not rows:
                    continue
                both = [r for r in rows if min(_tie_counts(sc[r], full[0][r], k)) >= 2]
                assert both, (shape, k, pat)
        # ... and the groups are spread over the id range (they straddle every slice of a 64-way cut)
        if N >= 1037:
            for r in range(n):
                if SC.pattern_of(r) == "eight":
                    t = SO.fold(sc[r])[full[0][r, 99]]
                    at = np.nonzero(SO.fold(sc[r]) == t)[0]
                    assert len(set((at * 64 // N).tolist())) >= 32, (shape, r)
        # the cluster row: the top-(k + 1) differ only below bit 10, for every k < 1024
        for r in range(n):
            if SC.pattern_of(r) == "cluster":
                assert len(np.unique(sc[r])) == N
                top = sc[r][full[0][r, :min(N, 1024)]].view(np.uint32)
                assert len(set((top >> 10).tolist())) == 1 and len(set(top.tolist())) == len(top)
        # special rows hold every special value
        for r in range(n):
            if SC.pattern_of(r) == "special" and N >= 1037:
                row = sc[r]
                assert np.isnan(row).any() and np.isposinf(row).any() and np.isneginf(row).any()
                assert ((row == 0) & np.signbit(row)).any() and ((row == 0) & ~np.signbit(row)).any()
                assert ((np.abs(row) > 0) & (np.abs(row) < 1.1754944e-38)).any()
        # exclusion lists: empty, covering the top entries, covering everything
        off, ids = F["ex"]
        ln = np.diff(off)
        assert (ln == 0).any() and (n < 8 or (ln == N).any())
        withl = SC.expected(shape, True)
        assert np.array_equal(withl[2], N - ln)
        if n >= 8:
            assert ((withl[0][:, 0] != full[0][:, 0]) & (full[0][:, 0] >= 0)).any()      # a list took the best entry away
    assert seen == set(SC.PATTERNS)
    assert {n for n, _ in SC.SHAPES.values()} == {1, 31, 32, 33, 70, 300} and {N for _, N in SC.SHAPES.values()} == {5, 13, 1037, 3000, 5000}
    assert 4096 in SC.ks_of(5000) and max(SC.ks_of(3000)) == 1025


def test_entry_points_are_declared_bound_and_built():
    import poi_amd
    from poi_amd import evaluate as E
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    for name, n_args in (("poi_score_rows", 17), ("poi_topk_select", 12), ("poi_score_candidates", 21)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/poi_hip.h" % name
        assert name in poi_amd._lib.SIGNATURES, "%s has no ctypes binding" % name
        assert len(poi_amd._lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == n_args, "%s: argument counts differ" % name
    assert re.search(r"additive to 9: candidate generation - new entry points poi_score_rows, poi_topk_select and poi_score_candidates", hdr)
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    assert "select.hip" in poi_amd.build.SOURCES
    for key in ("select_rows_per_chunk", "select_chunks", "select_path", "select_splits"):
        assert key in poi_amd._lib.PLAN_KEYS and '"%s"' % key in hdr
    for opt in ("select_split_max", "select_grid", "select_chunk_mb"):
        assert '"%s"' % opt in hdr
    for name in ('"score_rows"', '"topk_select"', '"score_candidates"'):
        assert name in hdr
    assert hasattr(poi_amd.models._Base, "compute_sub_candidates") and hasattr(poi_amd.models.Session, "candidates")
    assert hasattr(E, "candidate_recall")
