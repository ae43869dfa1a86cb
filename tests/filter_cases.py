"""The problems of tests/test_gpu_filter.py, built on the host: tests/test_filter_cpu.py checks on the CPU that they contain what they
claim (and that the oracle alone ranks the fused cases with clear gaps), the GPU tests feed them to the library.  Attribute tables and
predicates; planted float32 score rows (the patterns of tests/select_cases.py) with pass masks, per-row predicates and exclusion lists;
model cases from make_case of tests/test_gpu_near.py."""
import functools

import numpy as np

from tests import filter_oracle as FO
from tests import near_oracle as NO
from tests import select_cases as SC

N_ITEM, N_CAT = 1003, 37                             # no multiple of 32, of 64 or of a tile; category 36 has no POI, 35 a handful
N_ROWS = 70
K = 20

# what every predicate list of the build test exercises: no condition, one category, many, a category no POI has, need only, any only,
# forbid matching everything (bit 7 is set on every POI), everything combined, a category with three POIs
PREDICATES = [dict(), dict(categories=[3]), dict(categories=[0, 1, 2, 5, 8, 13, 21, 34]), dict(categories=[36]), dict(need=0b101),
              dict(any=0b11000), dict(forbid=0x80), dict(categories=[3, 4], need=1, forbid=2), dict(categories=[35]),
              dict(need=0x80000000), dict(categories=[7], any=0xFFFFFFFF)]
P_ALL, P_SPARSE, P_NONE = 0, 8, 3


@functools.lru_cache(maxsize=None)
def attributes(n_item=N_ITEM, strays=False):
    """(cat int32, flags uint32): very unequal category sizes over 0 .. 34, exactly three POIs of category 35 (far apart: most item
    tiles hold none), none of 36; flag bits 0 - 4 random, bit 7 on every POI, bit 31 on every fifth.  strays: five POIs get a category
    outside [0, N_CAT)."""
    rng = np.random.default_rng(4000 + n_item)
    w = 1.0 / np.arange(1, 36) ** 1.3
    cat = rng.choice(35, n_item, p=w / w.sum()).astype(np.int32)
    cat[[11, n_item // 2, n_item - 2]] = 35
    flags = (rng.integers(0, 32, n_item).astype(np.uint32) | np.uint32(0x80)
             | ((np.arange(n_item) % 5 == 0).astype(np.uint32) << np.uint32(31))).astype(np.uint32)
    if strays:
        cat[[0, 40, 41, n_item // 3, n_item - 1]] = [N_CAT, -1, 5000, -(2 ** 31), N_CAT + 1]
    return cat, flags


# ---- planted score rows for poi_topk_filtered_scores ---------------------------------------------------------------------------------
SCORE_SHAPES = {"odd": (33, 1003), "wide": (70, 4099)}
MASKS = ("all", "half", "few", "seven", "none")      # "few": 20 POIs pass (fewer than k = 32); "seven": fewer than any k > 7


@functools.lru_cache(maxsize=None)
def score_fixture(shape):
    """dict(sc (n, n_item) float32, pmask (5, n_item) bool, pred (n) int, ex (off, ids), bad (n) bool): row r holds pattern
    r % len(SC.PATTERNS) - plateaus and eight-value rows (ties straddling every K-th place), NaN / +-inf / +-0.0 / denormals, rows with
    nothing selectable - and uses one of the five masks; the last row plants zeros of both signs.  Two rows name a predicate outside [0, 5), one row's list descends, one leaves the
    table: the bad rows."""
    n, N = SCORE_SHAPES[shape]
    rng = np.random.default_rng(5000 + n + N)
    sc = np.stack([SC.pattern_row(SC.pattern_of(r), N, rng) for r in range(n)])
    pmask = np.zeros((len(MASKS), N), bool)
    pmask[0] = True
    pmask[1] = rng.random(N) < 0.5
    pmask[2, rng.choice(N, 20, replace=False)] = True
    pmask[3, rng.choice(N, 7, replace=False)] = True
    pred = (np.arange(n) // len(SC.PATTERNS) + np.arange(n)) % len(MASKS)      # (every pattern meets several masks)
    # the last row, on the mask that passes everything: +inf, five ones, then zeros of both signs in id order (the tie among them
    # straddles every K-th place beyond 6) between NaN and -inf entries
    z = rng.choice(np.array([0.0, -0.0, np.nan, -np.inf], np.float32), N)
    z[rng.choice(N, 6, replace=False)] = [np.inf, 1.0, 1.0, 1.0, 1.0, 1.0]
    sc[n - 1], pred[n - 1] = z, 0
    lists = []
    for r in range(n):
        kind = (r // len(MASKS)) % 3
        lists.append(np.zeros(0, np.int64) if kind == 0 else np.sort(rng.choice(N, rng.integers(1, 60), replace=False)) if kind == 1
                     else np.nonzero(pmask[pred[r]])[0][::2])      # kind 2: every second passing POI leaves
    lists[n - 1] = np.zeros(0, np.int64)
    bad = np.zeros(n, bool)
    pred[5], pred[12] = len(MASKS), -1
    lists[20] = np.array([9, 8, 7])
    lists[26] = np.array([3, N])
    bad[[5, 12, 20, 26]] = True
    return dict(sc=sc, pmask=pmask, pred=pred, ex=FO.csr(lists), bad=bad)


@functools.lru_cache(maxsize=None)
def score_expected(shape):
    """(ids, scores, counts) of a fixture at k = 32 with its lists; a shorter list is a prefix."""
    F = score_fixture(shape)
    mask, bad = FO.candidate_masks(F["pmask"], F["pred"], len(F["sc"]), *F["ex"])
    assert np.array_equal(bad, F["bad"])
    return FO.topk(F["sc"], mask, FO.K_MAX)


# ---- model cases for the fused paths ----------------------------------------------------------------------------------------------------
FUSED_CASES = [("bpr", 32), ("bpr", 64), ("bpr", 128), ("bpr", 256), ("spatial", 32), ("spatial", 64), ("spatial", 128), ("spatial", 256)]
ORACLE_SEEDS = {("bpr", 32): 700, ("spatial", 64): 701}      # the independence test's cases: seeds at which the oracle alone has clear gaps


@functools.lru_cache(maxsize=None)
def fused_case(kind, dim, seed=None, n_item=N_ITEM):
    """make_case over N_ROWS users and n_item POIs, with: pmask (the PREDICATES over attributes(n_item)), pred (a predicate per row,
    the sparse and the empty one among them), anchor (the users' last train POIs, -1 on rows 3 and 40), ex (one ascending list per
    row)."""
    from tests.test_gpu_near import last_of, make_case
    C = make_case(kind, dim, 600 + dim if seed is None else seed, n_user=N_ROWS, n_item=n_item)
    cat, flags = attributes(n_item)
    pmask, strays = FO.pass_mask(cat, flags, N_CAT, PREDICATES)
    assert strays == 0
    rng = np.random.default_rng(610 + dim)
    pred = rng.integers(0, len(PREDICATES), N_ROWS)
    pred[:6] = [P_ALL, P_SPARSE, P_NONE, 2, 4, 5]
    anchor = last_of(C["T"]).astype(np.int64)
    anchor[[3, 40]] = -1
    lists = [np.sort(rng.choice(n_item, rng.integers(0, 60), replace=False)) if r % 3 else np.zeros(0, np.int64) for r in range(N_ROWS)]
    return dict(C=C, cat=cat, flags=flags, pmask=pmask, pred=pred, anchor=anchor, ex=FO.csr(lists))


def oracle_scores(F):
    """float64 scores of a fused case (near_oracle.scores: the distance term at the anchor, none on a row without one)."""
    C, T = F["C"], F["C"]["T"]
    if C["term"] is None:
        return NO.scores(C["users"], C["items"])
    return NO.scores(C["users"], C["items"], F["anchor"], C["term"][0], C["term"][1], T["coords"], T["dd_m"], T["n_dist"])
