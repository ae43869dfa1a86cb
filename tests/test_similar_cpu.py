"""CPU tests of the similar-rows entries' host side: the oracle of tests/similar_oracle.py against a brute-force double loop, the launch
planner (csrc/similar_plan.h) compiled on its own at its switch points, header / export / binding agreement with the ABI still 9, the
host argument checks of models.similar_pois / similar_users / nearest_visited, evaluate.similar_covisit_rate on a hand-made dataset,
and the condition on the fixtures of tests/test_gpu_similar.py - at least 90 % of the queries of every ranking fixture have clear
top-(k + 1) gaps under the oracle alone, at least 90 % of the nearest-visited pairs a clear best-to-second gap.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import poi_amd
from poi_amd import evaluate as E, models as M
from tests import similar_cases as SC
from tests import similar_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_matches_a_brute_force():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (11, 4))
    x[6] = 0.0                                                                # a zero row: emb 0 against everything
    coords = np.c_[rng.uniform(40.0, 40.3, 11), rng.uniform(-74.2, -73.8, 11)]
    qs = [4, 0, 6, 4, 9]
    ex = [[1, 7], [], [0, 2], list(range(11)), [9]]                           # (query 3 excludes everything, itself included; query 4 itself alone)
    eo, ei = SO.csr(ex)
    for g, s in ((0.0, 1.0), (0.5, 5.0), (0.3, 1.0)):
        sim = SO.sim_matrix(x, coords, g, s)
        assert np.array_equal(sim, sim.T) or np.allclose(sim, sim.T, rtol=1e-15, atol=0)
        got = SO.topk(sim[qs], SO.candidate_mask(qs, 11, eo, ei), 5)
        want = SO.brute_force(x, coords, g, s, qs, 5, [set(e) for e in ex])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and want[2].tolist() == [8, 10, 8, 0, 10]
        assert np.allclose(got[1], want[1], rtol=1e-12, atol=1e-15)
        if g == 0.0:
            assert np.all(sim[6] == 0.0) and np.all(sim[:, 6] == 0.0)
    assert np.all(got[0][3] == -1) and np.all(np.isneginf(got[1][3]))
    inv = SO.inv_norms(x)
    assert inv[6] == 0.0 and np.allclose(inv[:6] * np.sqrt((x[:6] ** 2).sum(1)), 1.0, rtol=1e-15)


def test_nearest_oracle_on_a_hand_made_row():
    items = np.array([[1.0, 0, 0, 0], [0.9, 0.1, 0, 0], [0, 1.0, 0, 0], [1.0, 0, 0, 0], [0, 0, 0, 0]])
    lists = np.array([[0, 2, -1], [1, 4, 0]])
    off, ids = SO.csr([[2, 3, 1, 3], []])
    pos, sim, gap, twin = SO.nearest(lists, off, ids, items, None, 0.0, 1.0)
    assert pos.tolist() == [[1, 0, -1], [-1, -1, -1]] and sim[0, 0] == 1.0 and sim[0, 1] == 1.0 and np.isneginf(sim[0, 2]) and np.isneginf(sim[1]).all()
    assert gap[0, 0] == 0.0 and twin[0, 0] and gap[0, 1] > 0.5 and not twin[0, 1]      # POI 3 twice: a tie of one POI with itself


_MAIN = r"""
#include <stdio.h>
#include "similar_plan.h"
int main() {
  int n_q, n, k, rows_max, split_max, grid_opt, num_cu;
  long long rows_fit;
  while (scanf("%d %d %d %d %lld %d %d %d", &n_q, &n, &k, &rows_max, &rows_fit, &split_max, &grid_opt, &num_cu) == 8) {
    const SimilarPlan P = similar_plan(n_q, n, k, rows_max, rows_fit, split_max, grid_opt, num_cu);
    printf("%d %d\n", P.path, P.n_split);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("similar_plan")
    cxx = shutil.which("c++") or shutil.which("g++") or poi_amd.build._hipcc()
    src, exe = str(d / "similar_plan_main.cpp"), str(d / "similar_plan_main")
    open(src, "w").write(_MAIN)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", poi_amd.build.CSRC, src, "-o", exe], check=True)      # alone: no HIP anywhere near it

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        got = [tuple(int(v) for v in line.split()) for line in out if line]
        assert len(got) == len(cases)
        return got
    return run


def _plan(n_q, n, k, rows_max, rows_fit, split_max, grid_opt, num_cu):
    """The rule, re-spelled.  The walk's slices: at most split_max queries take them - the grid option as given, otherwise two
    workgroups per CU over the query blocks while a slice keeps 16 tiles; at least one, at most 64.  The route: at most rows_max
    queries go through the score rows while they fit and k <= n."""
    split, s = 0, 1
    if n_q <= split_max:
        split, s = 1, grid_opt
        if grid_opt <= 0:
            s = max(1, min(2 * num_cu // max((n_q + 31) // 32, 1), ((n + 31) // 32) // 16))
        s = min(s, 64)
    if n_q <= rows_max and n_q <= rows_fit and k <= n:
        return (2, s)
    return (split, s)


def test_the_plan_header_at_its_switch_points(planner):
    cases = [(n_q, n, k, rows_max, fit, split_max, grid, cu) for n_q in (1, 31, 32, 33, 256, 257, 100000) for n in (6, 300, 3001, 100000)
             for k in (1, 20, 32) for rows_max in (0, 32, 4096) for fit in (0, 32, 1 << 40) for split_max in (0, 256, 1 << 30) for grid in (0, 7, 64)
             for cu in (1, 256)]
    got = planner(cases)
    for c, g in zip(cases, got):
        assert g == _plan(*c), (c, g)
    named = {c: g for c, g in zip(cases, got)}
    big = 1 << 40
    assert named[(1, 100000, 20, 32, big, 256, 0, 256)] == (2, 64)            # one query: the score rows, their walk over 64 slices
    assert named[(32, 100000, 20, 32, big, 256, 0, 256)] == (2, 64) and named[(33, 100000, 20, 32, big, 256, 0, 256)] == (1, 64)      # the switch
    assert named[(1, 100000, 20, 0, big, 256, 0, 256)] == (1, 64)             # rows_max 0: never
    assert named[(32, 100000, 20, 32, 0, 256, 0, 256)] == (1, 64)             # the rows do not fit the workspace
    assert named[(1, 6, 20, 32, big, 256, 0, 256)] == (1, 1)                  # k > n: the selection cannot take the call
    assert named[(257, 100000, 20, 32, big, 256, 0, 256)] == (0, 1) and named[(256, 100000, 20, 32, big, 256, 0, 256)] == (1, 64)
    assert named[(33, 3001, 20, 32, big, 1 << 30, 7, 256)] == (1, 7) and named[(33, 3001, 20, 32, big, 0, 7, 256)] == (0, 1)


ENTRIES = {"poi_row_inv_norms": 6, "poi_similar_topk": 18, "poi_similar_rows": 14, "poi_similar_nearest": 16}


def test_header_exports_and_bindings_agree_and_the_abi_is_still_9():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    abi = open(os.path.join(poi_amd.build.CSRC, "abi_serve.hip")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, hdr, re.S)
        assert m, "%s is not declared in include/poi_hip.h" % name
        d = re.search(r"\nint %s\(([^{]*?)\) \{" % name, abi, re.S)
        assert d, "%s is not defined in csrc/abi_serve.hip" % name
        assert name in poi_amd._lib.SIGNATURES, "%s has no ctypes binding" % name
        assert len(poi_amd._lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == d.group(1).count(",") + 1 == n_args, name
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    assert "similar.hip" in poi_amd.build.SOURCES
    for key in ("similar_path", "similar_splits", "similar_split_max"):
        assert key in poi_amd._lib.PLAN_KEYS and '"%s"' % key in hdr
    for opt in ("similar_split_max", "similar_grid", "similar_rows_max"):
        assert '"%s"' % opt in hdr and '{"%s"' % opt in open(os.path.join(poi_amd.build.CSRC, "abi.hip")).read()
    for name in ("similar_topk", "similar_norms", "similar_walk", "similar_merge", "similar_rows", "similar_nearest"):
        assert '"%s"' % name in hdr
    plan = open(os.path.join(poi_amd.build.CSRC, "similar_plan.h")).read()
    assert re.search(r"#define SIMILAR_ROWS_MAX_DEFAULT (\d+)", plan).group(1) in re.search(r'"similar_rows_max" n \(default (\d+)', hdr).group(1)


def test_host_argument_checks():
    obj = M._Base()
    assert obj._similar_args(32, 6, 0.0, 1.0) == (32, 0.0, 1.0) and obj._similar_args(299, 300, 0.5, 5) == (299, 0.5, 5.0)
    assert obj._similar_args(4096, 5000, 0.99, 0.1)[0] == 4096
    for k, n in ((0, 300), (300, 300), (33, 33), (4097, 5000), (-1, 300)):
        with pytest.raises(ValueError, match="similar"):
            obj._similar_args(k, n, 0.0, 1.0)
    for g in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="geo_weight"):
            obj._similar_args(20, 300, g, 1.0)
    for s in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale_km"):
            obj._similar_args(20, 300, 0.5, s)
    obj.device = "cpu"
    assert obj._similar_queries([3, 0, 3], 5, "pois").tolist() == [3, 0, 3]
    for bad in ([5], [-1], [2, 7]):
        with pytest.raises(IndexError, match="pois"):
            obj._similar_queries(bad, 5, "pois")
    for g in (-0.1, 1.1):
        with pytest.raises(ValueError, match="geo_weight"):
            obj.nearest_visited([0], [[1]], geo_weight=g)
    with pytest.raises(ValueError, match="scale_km"):
        obj.nearest_visited([0], [[1]], scale_km=0.0)


class _Toy:
    """What evaluate.similar_covisit_rate reads of a model: the train CSR and similar_pois."""
    n_item = 6

    def __init__(self):
        import torch
        seqs = [[0, 1], [1, 2], [0, 1, 2], [3], [4, 5], [5, 6]]              # (6: a padding id, no visit)
        self._off_host = np.r_[0, np.cumsum([len(s) for s in seqs])]
        self.p = torch.as_tensor(np.concatenate(seqs).astype(np.int32))
        self.calls = []

    def similar_pois(self, pois, k, geo_weight=0.0, scale_km=1.0):
        import torch
        self.calls.append((len(pois), k, geo_weight, scale_km))
        table = {0: [1, 2], 1: [0, 2], 2: [1, 3], 3: [4, -1], 4: [5, 0], 5: [4, 3]}
        return torch.as_tensor(np.array([table[int(j)][:k] for j in pois], np.int32))


def test_similar_covisit_rate_on_a_hand_made_dataset():
    m = _Toy()
    out = E.similar_covisit_rate(m, 2, geo_weight=0.5, scale_km=3.0)
    # visitors: 0 {0, 2}, 1 {0, 1, 2}, 2 {1, 2}, 3 {3}, 4 {4}, 5 {4, 5}.  Pairs that share one: (0,1) (0,2) (1,0) (1,2) (2,1) (4,5) (5,4);
    # (2,3) (3,4) (4,0) (5,3) share none; the -1 of POI 3 is no pair
    assert m.calls == [(6, 2, 0.5, 3.0)] and out["pairs"] == 11 and out["similar"] == pytest.approx(7 / 11)
    assert 0.0 <= out["random"] <= 1.0 and out == E.similar_covisit_rate(m, 2, geo_weight=0.5, scale_km=3.0)      # (a fixed seed)
    from poi_amd import data as D
    vo, vu = D.visitors_csr(m._off_host, m.p.numpy(), 6)
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 6, 50), rng.integers(0, 6, 50)
    assert E._covisit_share(vo, vu, a, b) == pytest.approx(SO.covisit_share(vo, vu, a, b))


def test_ranking_fixtures_have_clear_gaps():
    for name, sc, mask in SC.fixtures():
        ok = SO.qualifying(sc, mask, SC.K)
        print("%s: %.1f %% of %d queries qualify, candidates %d..%d" % (name, 100 * ok.mean(), len(ok), mask.sum(axis=1).min(), mask.sum(axis=1).max()))
        assert len(sc) == SC.N_QUERY and (~mask).any(axis=1).all(), name
        assert ok.mean() >= 0.9, "%s: only %.1f %% of the queries have clear gaps: pick another seed" % (name, 100 * ok.mean())


def test_nearest_fixtures_have_clear_gaps():
    for kind, dim in (("bpr", 20), ("spatial", 128)):
        N = SC.nearest_case(kind, dim)
        R = N["R"]
        for hist in ("train", "own"):
            for g, s in ((0.0, 1.0), (0.5, 5.0), (1.0, 5.0)):
                pos, sim, gap, twin = SO.nearest(N["lists"], *N[hist], R["items"], R["coords"], g, s)
                live = pos >= 0
                ok = (gap >= 1e-9) | twin
                print("%s dim %d %s g %g: %.1f %% of %d pairs qualify" % (kind, dim, hist, g, 100 * ok[live].mean(), live.sum()))
                assert live.sum() > 1000 and ok[live].mean() >= 0.9, (kind, dim, hist, g)
                assert np.abs(sim[live]).max() <= 1.0 + 1e-12
