"""CPU-only tests of the filtered recommendation: the numpy oracle (tests/filter_oracle.py) on hand-made cases, the fixtures of
tests/filter_cases.py contain what they claim, data.pack_pass_bits and data.synthetic_attributes, the path rule of csrc/filter_plan.h
compiled on its own, and the header / binding declarations.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D
from tests import filter_cases as FC
from tests import filter_oracle as FO
from tests import near_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc")
INF, NAN = np.float32(np.inf), np.float32(np.nan)


# ---- the oracle on hand-made cases -------------------------------------------------------------------------------------------------------
def test_pass_mask_by_hand():
    cat = np.array([0, 1, 2, 1, 3, 9, -1], np.int32)      # n_cat = 4: POIs 5 and 6 are strays
    flags = np.array([0b000, 0b001, 0b011, 0b101, 0b111, 0b001, 0b001], np.uint32)
    preds = [dict(), dict(categories=[1]), dict(categories=[1, 3], need=0b001), dict(any=0b110), dict(forbid=0b001), dict(need=0b101, forbid=0b010),
             dict(categories=[2], any=0b100)]
    m, strays = FO.pass_mask(cat, flags, 4, preds)
    assert strays == 2
    assert m.astype(int).tolist() == [[1, 1, 1, 1, 1, 1, 1],      # no list: the strays pass
                                      [0, 1, 0, 1, 0, 0, 0],
                                      [0, 1, 0, 1, 1, 0, 0],
                                      [0, 0, 1, 1, 1, 0, 0],
                                      [1, 0, 0, 0, 0, 0, 0],
                                      [0, 0, 0, 1, 0, 0, 0],
                                      [0, 0, 0, 0, 0, 0, 0]]
    m1, _ = FO.pass_mask(cat, None, 4, [dict(), dict(need=1), dict(forbid=1), dict(any=1)])      # NULL flags read as zeros
    assert m1.all(axis=1).tolist() == [True, False, True, False] and not m1[1].any() and not m1[3].any()


def test_bits_by_hand():
    mask = np.zeros((2, 70), bool)
    mask[0, [0, 31, 32, 69]] = True
    mask[1] = True
    w = FO.bits(mask, ldw=4)
    assert w.dtype == np.uint32 and w.shape == (2, 4)
    assert w[0].tolist() == [0x80000001, 0x00000001, 0x00000020, 0]
    assert w[1].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x0000003F, 0]      # nothing at j >= 70
    assert np.array_equal(FO.unpack(w, 70), mask)


def test_topk_by_hand():
    #            0    1     2    3     4     5    6     7     8
    sc = np.array([[1.0, 2.0, 2.0, NAN, -INF, INF, -0.0, 0.0, 2.0]], np.float32)
    mask = np.ones((1, 9), bool)
    ids, val, cnt = FO.topk(sc, mask, 8)
    assert ids.tolist() == [[5, 1, 2, 8, 0, 6, 7, -1]] and cnt.tolist() == [9]      # ties by id; both zeros one score; NaN / -inf never listed
    assert val[0, :7].tolist() == [INF, 2.0, 2.0, 2.0, 1.0, 0.0, 0.0] and np.isneginf(val[0, 7])
    assert not np.signbit(val[0, 5]) and not np.signbit(val[0, 6])                    # -0.0 comes out as +0.0
    mask[0, [1, 5]] = False
    ids, val, cnt = FO.topk(sc, mask, 3)
    assert ids.tolist() == [[2, 8, 0]] and cnt.tolist() == [7]                        # the count is |C|, not the selectable ones, not clipped
    ids, val, cnt = FO.topk(sc, np.zeros((1, 9), bool), 2)
    assert ids.tolist() == [[-1, -1]] and np.isneginf(val).all() and cnt.tolist() == [0]


def test_candidate_masks_by_hand():
    pmask = np.array([[1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 0, 1]], bool)
    ex_off, ex = FO.csr([[1, 3], [], [3, 1], [0, 6], [5], []])
    radius = np.ones((6, 6), bool); radius[1, :3] = False
    mask, bad = FO.candidate_masks(pmask, [0, 1, 0, 0, 2, 1], 6, ex_off, ex, anchor=[0, 3, -1, 2, 0, 6], radius_mask=radius)
    assert bad.tolist() == [False, False, True, True, True, True]      # descending list, id outside the table, predicate 2 of 2, anchor 6 of 6
    assert mask[0].tolist() == [True, False, True, False, True, True]
    assert mask[1].tolist() == [False, False, False, True, False, True]
    assert not mask[2:].any()


def test_the_anchor_is_a_candidate_only_if_it_passes():
    xy = np.array([[40.0, -74.0], [40.0, -74.0], [41.0, -74.0]])
    radius = NO.candidate_mask(xy, [0, 1], 0.0)                        # radius 0: the anchor and what shares its coordinates
    assert radius.tolist() == [[True, True, False], [True, True, False]]
    mask, bad = FO.candidate_masks(np.array([[False, True, True]]), None, 2, anchor=[0, 1], radius_mask=radius)
    assert not bad.any() and mask.tolist() == [[False, True, False], [False, True, False]]


# ---- the fixtures contain what they claim ----------------------------------------------------------------------------------------------
def test_attribute_fixture():
    cat, flags = FC.attributes()
    assert len(cat) == FC.N_ITEM and FC.N_ITEM % 32 and cat.min() >= 0 and cat.max() == 35
    pm, strays = FO.pass_mask(cat, flags, FC.N_CAT, FC.PREDICATES)
    cnt = pm.sum(axis=1)
    assert strays == 0 and cnt[FC.P_ALL] == FC.N_ITEM and cnt[FC.P_NONE] == 0 and cnt[FC.P_SPARSE] == 3 and cnt[6] == 0
    assert 0 < cnt[1] < cnt[2] < FC.N_ITEM and 0 < cnt[4] < FC.N_ITEM and 0 < cnt[5] < FC.N_ITEM and cnt[9] == (FC.N_ITEM + 4) // 5
    tiles = np.add.reduceat(pm[FC.P_SPARSE], np.arange(0, FC.N_ITEM, 32))
    assert (tiles == 0).mean() > 0.9                                   # the sparse predicate leaves most item tiles empty
    c2, _ = FC.attributes(strays=True)
    assert FO.pass_mask(c2, flags, FC.N_CAT, FC.PREDICATES)[1] == 5


@pytest.mark.parametrize("shape", list(FC.SCORE_SHAPES))
def test_score_fixture(shape):
    F = FC.score_fixture(shape)
    ids, val, cnt = FC.score_expected(shape)
    n, N = F["sc"].shape
    assert (cnt[F["bad"]] == 0).all() and (ids[F["bad"]] == -1).all() and F["bad"].sum() == 4
    good = ~F["bad"]
    assert (cnt[good & (F["pred"] == 4)] == 0).all() and (cnt[good & (F["pred"] == 0)] > 32).any()
    short = good & (cnt > 0) & (ids[:, -1] == -1)
    assert short.any()                                                 # rows with fewer than k selectable passing POIs
    # ties straddle the K-th place: on a plateau row the 20th and the 21st entry share a score
    r = next(r for r in range(n) if good[r] and FC.SC.pattern_of(r) == "plateau" and cnt[r] > 32)
    assert val[r, 19] == val[r, 20] and ids[r, 19] < ids[r, 20]
    # both zeros and +inf are among the listed scores, and no listed zero is negative
    listed = val[ids >= 0]
    assert np.isposinf(listed).any() and (listed == 0).any() and not np.signbit(listed[listed == 0]).any()
    assert not np.isnan(listed).any() and not np.isneginf(listed).any()


def test_the_oracle_alone_ranks_the_independence_cases_with_clear_gaps():
    """The seeds of FC.ORACLE_SEEDS: at least 90 % of the rows have clear gaps among their candidates, with and without the radius."""
    for (kind, dim), seed in FC.ORACLE_SEEDS.items():
        F = FC.fused_case(kind, dim, seed)
        osc = FC.oracle_scores(F)
        T = F["C"]["T"]
        for r_km in (None, 8.0):
            radius = None if r_km is None else NO.candidate_mask(T["coords"], F["anchor"], r_km)
            mask, bad = FO.candidate_masks(F["pmask"], F["pred"], FC.N_ROWS, *F["ex"], anchor=F["anchor"], radius_mask=radius)
            assert not bad.any()
            ok = NO.qualifying(osc, mask, FC.K)
            assert ok.mean() >= 0.9, (kind, dim, r_km, ok.mean())


# ---- data.pack_pass_bits / data.synthetic_attributes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_item", [1, 31, 32, 33, 64, 1003, 4099])
def test_pack_pass_bits_is_the_oracle(n_item):
    import torch
    rng = np.random.default_rng(n_item)
    mask = rng.random((3, n_item)) < 0.3
    mask[1] = True
    W = (n_item + 31) // 32
    want = FO.bits(mask)
    got = D.pack_pass_bits(mask)
    assert got.dtype == np.uint32 and got.shape == (3, W) and np.array_equal(got, want)
    assert np.array_equal(D.pack_pass_bits(mask, ldw=W + 2), FO.bits(mask, ldw=W + 2))
    assert np.array_equal(D.pack_pass_bits(mask[0]), want[:1])        # one predicate
    t = D.pack_pass_bits(torch.as_tensor(mask))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        D.pack_pass_bits(mask, ldw=W - 1)


def test_synthetic_attributes():
    cat, flags = D.synthetic_attributes(100000, 200, seed=3)
    assert cat.dtype == np.int32 and flags.dtype == np.uint32 and cat.shape == flags.shape == (100000,)
    assert cat.min() >= 0 and cat.max() < 200
    size = np.bincount(cat, minlength=200)
    assert size.max() > 50 * max(1, np.sort(size)[100])                # very unequal: the largest against the median category
    frac = [float(((flags >> b) & 1).mean()) for b in (0, 1, 4)]
    assert 0.45 < frac[0] < 0.55 and 0.08 < frac[1] < 0.12 and 0.005 < frac[2] < 0.02
    c2, f2 = D.synthetic_attributes(100000, 200, seed=3)
    assert np.array_equal(cat, c2) and np.array_equal(flags, f2)


# ---- csrc/filter_plan.h on its own -----------------------------------------------------------------------------------------------------
_PLAN_MAIN = r"""
#include "filter_plan.h"
#include <stdio.h>
int main() {
  long long a[6];
  while (scanf("%lld %lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5) == 6)
    printf("%d\n", plan_filter_path((int)a[0], a[1] != 0, a[2], a[3], a[4], a[5]));
  printf("%d %d %d %d\n", FILTER_PATH_AUTO, FILTER_PATH_WALK, FILTER_PATH_GATHER, FILTER_GATHER_COST_DEFAULT);
  return 0;
}
"""


def test_filter_plan_compiles_alone_and_follows_the_rule(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or poi_amd.build._hipcc()
    src, exe = str(tmp_path / "filter_plan_main.cpp"), str(tmp_path / "filter_plan_main")
    open(src, "w").write(_PLAN_MAIN)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, src, "-o", exe], check=True)
    AUTO, WALK, GATHER = 0, 1, 2
    G = 8
    # (requested, radius, n, n_item, cand_hint, G) -> path
    cases = [((AUTO, 1, 4096, 100000, 0, G), GATHER),                 # a finite radius: gather, whatever the hint
             ((AUTO, 1, 1, 100000, 100000, G), GATHER),
             ((AUTO, 0, 64, 100000, 0, G), WALK),                     # hint 0 = unknown: walk
             ((AUTO, 0, 1, 100000, 12499, G), GATHER),                # 1 * 12499 * 8 = 99992 < 1 * 100000
             ((AUTO, 0, 1, 100000, 12500, G), WALK),                  # 100000 < 100000 is false
             ((AUTO, 0, 64, 100000, 390, G), GATHER),                 # 64 * 390 * 8 = 199680 < 2 * 100000
             ((AUTO, 0, 64, 100000, 391, G), WALK),                   # 200192
             ((AUTO, 0, 4096, 100000, 390, G), GATHER),               # 128 tiles: 12779520 < 12800000
             ((AUTO, 0, 4096, 100000, 391, G), WALK),
             ((AUTO, 0, 33, 1003, 7, G), GATHER),                     # 33 * 7 * 8 = 1848 < 2 * 1003
             ((AUTO, 0, 33, 1003, 8, G), WALK),
             ((AUTO, 0, 64, 100000, 390, 9), WALK),                   # the same call under a dearer gather
             ((AUTO, 0, 4096, 2000000000, 1000000000, 1), WALK),      # 64-bit products: 4.096e12 < 2.56e11 is false
             ((AUTO, 0, 4096, 2000000000, 62499999, 1), GATHER),      # 2.55999995904e11 < 2.56e11
             ((WALK, 0, 1, 100000, 1, G), WALK), ((GATHER, 0, 4096, 100000, 100000, G), GATHER), ((GATHER, 1, 1, 10, 0, G), GATHER)]
    text = "".join("%d %d %d %d %d %d\n" % c for c, _ in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [int(v) for v in out[:len(cases)]]
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g, want)
    assert out[len(cases)].split()[:3] == ["0", "1", "2"]
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert re.search(r"POI_FILTER_AUTO = 0, POI_FILTER_WALK = 1, POI_FILTER_GATHER = 2", hdr)


# ---- declarations -------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "/* additive to 9: filtered recommendation - new entry points poi_filter_build, poi_score_topk_filtered and poi_topk_filtered_scores" in flat
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("poi_filter_build", 15), ("poi_score_topk_filtered", 29), ("poi_topk_filtered_scores", 16)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == n_args, name
        assert name in poi_amd._lib.SIGNATURES and len(poi_amd._lib.SIGNATURES[name][1]) == n_args, name
    for key in ("filter_path", "filter_splits", "filter_split_max"):
        assert key in poi_amd._lib.PLAN_KEYS
    src = open(os.path.join(CSRC, "abi.hip")).read()
    for opt in ("filter_split_max", "filter_grid", "filter_gather_cost"):
        assert '"%s"' % opt in src, opt
    assert "filter.hip" in poi_amd.build.SOURCES
