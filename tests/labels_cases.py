"""The problems of tests/test_gpu_labels.py, built on the host: tests/test_labels_cpu.py checks on the CPU that they contain what
they claim (and that the float64 oracle alone leaves at least 90 % of their rows clear), the GPU tests feed them to the library.
Random uniform(-0.5, 0.5) tables with labellings of 1 .. 1681 labels, with and without the distance term (11 and 200 bins), a 12-POI
problem worked by hand, a planted problem on which the mass and the max order differ, and planted exact tables with ties."""
import functools

import numpy as np

from tests import filter_oracle as FO
from tests import labels_oracle as LO

N_ROWS = 144                                          # four and a half 32-row tiles
BOX_KM = 40.0

# name -> (n_item, n_label, labelling, dim, k, distance bins or 0): the shapes of the issue's clear-row check, then the small and
# the spatial ones (n_item no multiple of 32; one label; 200 bins; a 27-POI table of less than one tile)
CASES = {
    "cat37": (2100, 37, "uniform", 32, 10, 0),
    "zipf37": (2100, 37, "zipf", 128, 20, 0),
    "many700": (2100, 700, "uniform", 64, 20, 0),
    "five": (1003, 5, "uniform", 16, 5, 0),
    "grid1681": (2100, 1681, "grid", 128, 32, 0),
    "wide256": (1003, 37, "zipf", 256, 10, 0),
    "one": (1003, 1, "uniform", 32, 1, 0),
    "tiny27": (27, 5, "uniform", 16, 5, 11),
    "geo11": (1003, 37, "zipf", 64, 10, 11),
    "geo200": (2100, 37, "mixed", 32, 10, 200),
}
# name -> a pinned seed (default: 9000 + the sum of the name's characters).  32 labels of one or two POIs each need 33 clear gaps per
# row: the seed is one at which the float64 oracle ALONE leaves 93 % of the rows clear (test_labels_cpu.py holds every case to 90 %)
SEEDS = {"grid1681": 9206}


def box_coords(rng, n_item):
    return np.stack((30.0 + rng.uniform(0, BOX_KM / 111.0, n_item), 120.0 + rng.uniform(0, BOX_KM / 96.0, n_item)), axis=1)


def labelling(kind, n_item, n_label, rng, coords):
    """(n_item) int32 labels below n_label; "mixed": every seventh POI unlabelled (several negative values)."""
    j = np.arange(n_item)
    if kind == "uniform":
        lab = rng.integers(0, n_label, n_item)
    elif kind in ("zipf", "mixed"):                   # very unequal sizes; the last label has no POI at all
        w = 1.0 / np.arange(1, n_label) ** 1.3
        lab = rng.choice(n_label - 1, n_item, p=w / w.sum())
        if kind == "mixed":
            lab = np.where(j % 7 == 3, -1 - (j % 5), lab)
    elif kind == "grid":                              # a 41 x 41 grid over the box: 1681 cells, clustered in space, most of them with one or two POIs
        side = int(round(n_label ** 0.5))
        assert side * side == n_label
        gy = np.minimum((coords[:, 0] - 30.0) / (BOX_KM / 111.0) * side, side - 1).astype(np.int64)
        gx = np.minimum((coords[:, 1] - 120.0) / (BOX_KM / 96.0) * side, side - 1).astype(np.int64)
        lab = gy * side + gx
    else:
        raise KeyError(kind)
    return lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(users (N_ROWS, dim) float32, items (n_item + 1, dim) float32 (the last row is the padding row), labels, n_label, k, ex (off,
    ids): an ascending list on two rows of three, and geo = None or dict(coords, cphi, thr, sts, wd, anchor, n_dist, dd_m); anchors -1
    on rows 3 and 40)."""
    from poi_amd import data
    n_item, n_label, kind, dim, k, n_dist = CASES[name]
    rng = np.random.default_rng(SEEDS.get(name, 9000 + sum(map(ord, name))))
    users = rng.uniform(-0.5, 0.5, (N_ROWS, dim)).astype(np.float32)
    items = rng.uniform(-0.5, 0.5, (n_item + 1, dim)).astype(np.float32)
    coords = box_coords(rng, n_item)
    labels = labelling(kind, n_item, n_label, rng, coords)
    lists = [np.sort(rng.choice(n_item, rng.integers(0, min(60, n_item)), replace=False)) if r % 3 else np.zeros(0, np.int64) for r in range(N_ROWS)]
    geo = None
    if n_dist:
        dd_m = 30000.0 / n_dist
        e = np.exp(rng.uniform(-2, 2, (N_ROWS, n_dist + 1)))
        anchor = rng.integers(0, n_item, N_ROWS)
        anchor[[3, 40]] = -1
        geo = dict(coords=coords, cphi=data.cos_lat(coords), thr=data.bin_thresholds(dd_m, n_dist), sts=(e / e.sum(axis=1, keepdims=True)).astype(np.float32),
                   wd=np.float32(0.7), anchor=anchor, n_dist=n_dist, dd_m=dd_m)
    return dict(name=name, users=users, items=items, labels=labels, n_label=n_label, k=k, n_item=n_item, dim=dim, ex=FO.csr(lists), geo=geo)


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """float64 scores (N_ROWS, n_item) of a case from its float32 tables (near_oracle.scores: the distance term at the anchor, none on
    a row without one)."""
    from tests import near_oracle as NO
    C = case(name)
    g = C["geo"]
    if g is None:
        return NO.scores(C["users"], C["items"])
    return NO.scores(C["users"], C["items"], g["anchor"], float(g["wd"]), g["sts"], g["coords"], g["dd_m"], g["n_dist"])


def ex_mask(C, rows=None, ex="own"):
    """(rows, n_item) bool candidate masks of a case under its own lists (or `ex`, or none)."""
    rows = np.arange(N_ROWS) if rows is None else np.asarray(rows)
    exl = sub_lists(C["ex"], rows) if isinstance(ex, str) else ex
    mask, bad = FO.candidate_masks(np.ones((1, C["n_item"]), bool), None, len(rows), *(exl if exl is not None else (None, None)))
    assert not bad.any()
    return mask


def sub_lists(ex, rows):
    return FO.csr([ex[1][ex[0][r]:ex[0][r + 1]] for r in rows])


# ---- the problem worked by hand ---------------------------------------------------------------------------------------------------------
# 12 POIs; labels A = 0 (ids 0 - 3), B = 1 (4 - 6), C = 2 (7 - 10), id 11 unlabelled; label 3 has no POI.  Scores are multiples of
# log 2 below the maximum 0, so every exp is a power of two and every q an exact integer: with u = 2^36,
#   A: 0, -1, -1, -2  -> u (1 + 1/2 + 1/2 + 1/4) = 9/4 u      best 0 (score 0)
#   B: 0, -3, -3      -> u (1 + 1/8 + 1/8)       = 5/4 u      best 4 (score 0: ties A's best, the higher id)
#   C: -1, -1, -1, -1 -> u (4 / 2)               = 2 u        best 7 (-log 2; a tie of four inside the label)
#   rest: -2          -> u / 4
# total = 23/4 u.  By mass: A, C, B.  By max: A (0, id 0), B (0, id 4), C.  Excluding POI 0: A = 5/4 u ties B in mass -> A (lower label),
# and A's best becomes POI 1.
LN2 = float(np.log(2.0))
HAND_LABELS = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, -1], np.int32)
HAND_STEPS = np.array([0, -1, -1, -2, 0, -3, -3, -1, -1, -1, -1, -2])
HAND_SCORES = (HAND_STEPS * LN2)[None, :]
HAND_N_LABEL = 4
HAND_MASS_QUARTERS = [9, 5, 8, 0, 1]                  # mass_q / (u / 4) per bucket (label 3 empty, bucket 4 = unlabelled)
HAND_BEST = [0, 4, 7, -1, 11]
HAND_COUNT = [4, 3, 4, 0, 1]
HAND_ORDER = {"mass": [0, 2, 1], "max": [0, 1, 2]}


# ---- a planted problem where the two orders differ -----------------------------------------------------------------------------------------
def planted_orders(n_item=1003, n_label=5, cafes=400):
    """(scores (1, n_item) float64, labels): label 0 holds `cafes` POIs of score 1.0 ("decent cafes"), label 1 a single POI of score 3.0
    ("one excellent museum"), the others one POI each at 0.5 and below.  exp(3) = 20.1 < 400 exp(1) = 1087: by mass label 0 leads, by
    max label 1."""
    sc = np.full((1, n_item), -30.0)
    lab = np.full(n_item, -1, np.int32)
    lab[:cafes], sc[0, :cafes] = 0, 1.0
    lab[cafes], sc[0, cafes] = 1, 3.0
    for i, l in enumerate(range(2, n_label)):
        lab[cafes + 1 + i], sc[0, cafes + 1 + i] = l, 0.5 - i
    return sc, lab


# ---- planted exact tables: users[r] = e_r, items[j][r] = a small integer, so that the float32 product is exact --------------------------
PLANT_DIM = 32


@functools.lru_cache(maxsize=None)
def tie_tables(n_item=1003, n_label=7):
    """(users (32, 32), items (n_item + 1, 32), scores (32, n_item) float32, labels): row r ranks integer scores of 2 + r % 7 distinct
    values - ties in the best score inside and across every label, and, the masses being sums of few distinct integers' q, ties in
    mass; rows 28 - 31 hold zeros of both signs; item 5 holds a NaN and item 6 a -inf in column 27 - through the product POI 5 is NaN on
    every row, POI 6 -inf on row 27 and NaN elsewhere; labels j % n_label with every ninth POI unlabelled."""
    rng = np.random.default_rng(9100 + n_item)
    items = np.zeros((n_item + 1, PLANT_DIM), np.float32)
    for r in range(PLANT_DIM):
        items[:n_item, r] = rng.integers(-1, 1 + r % 7, n_item)
        if r >= 28:
            items[:n_item][rng.random(n_item) < 0.3, r] = -0.0
    items[5, 27], items[6, 27] = np.nan, -np.inf
    lab = (np.arange(n_item) % n_label).astype(np.int32)
    lab[::9] = -1
    # rows 0 and 1 of label pairs (0, 1): the same multiset of scores in both labels -> equal mass_q, the lower label first
    a, b = np.nonzero(lab == 0)[0], np.nonzero(lab == 1)[0]
    m = min(len(a), len(b))
    items[b[:m], 0] = items[a[:m], 0]
    items[b[m:], 0] = -1
    items[a[m:], 0] = -1
    users = np.eye(PLANT_DIM, dtype=np.float32)
    with np.errstate(invalid="ignore"):               # (0 x NaN and 0 x -inf are NaN: POIs 5 and 6 are NaN on every other row, as in the product)
        sc = (np.float64(users) @ np.float64(items[:n_item]).T).astype(np.float32)
    return users, items, sc, lab
