"""The problems of tests/test_gpu_capped.py, built on the host: tests/test_capped_cpu.py checks on the CPU that they contain what they
claim, the GPU tests feed them to the library.  Labelings over the POIs of tests/filter_cases.py, a 12-POI problem worked by hand, the
planted problem on which the "best 2 k of the union, then cap" shortcut is wrong, planted POI tables whose float32 products are exact
(ties, and the adversarial merge case), and the seeds of the independence test."""
import functools

import numpy as np

from tests import capped_oracle as CO
from tests import filter_cases as FC

K_SET = (1, 7, 20, 32)
PER_SET = (1, 2, 3, 32)
GRIDS = (1, 2, 3, 7, 64)
LABELINGS = ("one", "distinct", "three", "zipf", "mixed", "by id")


@functools.lru_cache(maxsize=None)
def labeling(name, n_item):
    """(labels int32 (n_item), n_label)."""
    j = np.arange(n_item)
    if name == "one":
        lab = np.zeros(n_item, np.int64)
    elif name == "distinct":
        lab = j
    elif name == "three":
        lab = np.random.default_rng(7000 + n_item).integers(0, 3, n_item)
    elif name == "zipf":
        lab = FC.attributes(n_item)[0].astype(np.int64)                       # 35 categories of very unequal size, one with three POIs
    elif name == "mixed":
        lab = np.where(j % 7 == 3, -1 - (j % 5), FC.attributes(n_item)[0])      # every seventh POI unlabelled (several negative values)
    elif name == "by id":
        lab = j * 8 // n_item                                                 # clustered by id: a wave's quarter of a slice holds one or two
    else:
        raise KeyError(name)
    return lab.astype(np.int32), int(max(lab.max() + 1, 1))


# ---- the problem worked by hand ---------------------------------------------------------------------------------------------------------
# 12 POIs; labels A = 0 (ids 0 - 3), B = 1 (4 - 6), C = 2 (7 - 10), id 11 unlabelled.  By better(): 0, 1, 4 (all 9: a tie inside A and
# across A / B), 2, 7, 11, 5, 8 (both 6: a tie across B / C), 3, 9, 6, 10.
HAND_LABELS = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, -1], np.int32)
HAND_SCORES = np.array([[9, 9, 8, 5, 9, 6, 3, 7, 6, 4, 2, 6.5]], np.float32)
HAND_WANT = {1: [0, 4, 7, 11], 2: [0, 1, 4, 7, 11, 5, 8]}                      # per -> the list at any k >= its length; shorter k: a prefix


# ---- the shortcut that is wrong ----------------------------------------------------------------------------------------------------------
def planted_shortcut_problem():
    """(scores (10), labels (10), slices, per, k): five slices of two POIs; POI 2 i carries label 0 and score 100 - i, POI 2 i + 1 label
    i + 1 and score 10 + i.  Every slice's capped top-2 is both of its POIs; the best 4 of their union are four POIs of label 0, which
    one cap cuts to ONE entry - the answer is [0, 9]."""
    i = np.arange(5)
    sc, lab = np.zeros(10, np.float32), np.zeros(10, np.int32)
    sc[2 * i], sc[2 * i + 1] = 100 - i, 10 + i
    lab[2 * i + 1] = i + 1
    return sc, lab, [np.array([2 * s, 2 * s + 1]) for s in range(5)], 1, 2


def slice_lists(sc, labels, slices, per, k):
    """Every slice's own capped top-k as (score, id) lists."""
    return [CO.recap([(float(sc[j]), int(j)) for j in s], labels, per, k) for s in slices]


def cuts(n_item, n_slice, strided):
    j = np.arange(n_item)
    return [j[s::n_slice] for s in range(n_slice)] if strided else [j[n_item * s // n_slice:n_item * (s + 1) // n_slice] for s in range(n_slice)]


# ---- planted POI tables: users[r] = e_r, items[j][r] = a small integer, so that the float32 product is exact -------------------------
PLANT_DIM = 32
PLANT_N_ITEM = 4099


@functools.lru_cache(maxsize=None)
def tie_tables(n_item=1003):
    """(users (32, 32), items (n_item, 32), scores (32, n_item)): row r ranks integer scores of 2 + r % 7 distinct values - ties across and
    inside every label, straddling the k-th place and the per-th place of a label; rows 28 - 31 hold zeros of both signs."""
    rng = np.random.default_rng(7100 + n_item)
    items = np.zeros((n_item, PLANT_DIM), np.float32)
    for r in range(PLANT_DIM):
        items[:, r] = rng.integers(-1, 1 + r % 7, n_item)
        if r >= 28:
            items[rng.random(n_item) < 0.3, r] = -0.0
    return np.eye(PLANT_DIM, dtype=np.float32), items, items.T.copy()


def merge_labels(n_item=PLANT_N_ITEM):
    return (np.arange(n_item) % 64).astype(np.int32)


@functools.lru_cache(maxsize=None)
def merge_tables(n_item=PLANT_N_ITEM):
    """(users, items, scores (len(GRIDS), n_item)): row i is planted for S = GRIDS[i] slices of the kernel's tile cut (slice s = the
    32-POI tiles ntile s // S .. ntile (s + 1) // S): with labels j % 64, label L's best POI (100000 - 1000 L) lies in slice L % S,
    and every other slice holds a near-best POI of the label (1 + s below the best); everything else is far below.  k = 32, per = 1:
    the answer is the best POI of the labels 0 .. 31, while the best 64 of the slices' lists are the copies of the first labels."""
    ntile = (n_item + 31) // 32
    lab = merge_labels(n_item)
    items = np.zeros((n_item, PLANT_DIM), np.float32)
    for i, S in enumerate(GRIDS):
        col = -1.0 - (np.arange(n_item) % 997)
        for s in range(S):
            lo, hi = 32 * (ntile * s // S), min(32 * (ntile * (s + 1) // S), n_item)
            for L in range(64):
                js = np.nonzero(lab[lo:hi] == L)[0]
                if len(js):
                    col[lo + js[0]] = 100000 - 1000 * L - (0 if s == L % S else 1 + s)
        items[:, i] = col
    users = np.zeros((len(GRIDS), PLANT_DIM), np.float32)
    users[np.arange(len(GRIDS)), np.arange(len(GRIDS))] = 1.0
    return users, items, items[:, :len(GRIDS)].T.copy()


# ---- the independence test: seeds at which the float64 oracle ALONE leaves at least 90 % of the rows qualifying ------------------------
ORACLE_SEEDS = {("bpr", 32): 700, ("spatial", 64): 701}
ORACLE_PERS = (1, 2)


def oracle_case(kind, dim):
    """(fused case, float64 scores, candidate masks, labels): filter_cases.fused_case at the pinned seed with its per-row predicates,
    anchors and exclusion lists, and the Zipf categories as labels."""
    from tests import filter_oracle as FO
    F = FC.fused_case(kind, dim, ORACLE_SEEDS[(kind, dim)])
    mask, bad = FO.candidate_masks(F["pmask"], F["pred"], FC.N_ROWS, *F["ex"], anchor=F["anchor"])
    assert not bad.any()
    return F, FC.oracle_scores(F), mask, labeling("zipf", FC.N_ITEM)[0]
