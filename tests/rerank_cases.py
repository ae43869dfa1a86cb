"""The candidate lists of tests/test_gpu_rerank.py, built on the host: tests/test_rerank_cpu.py checks under the oracle alone
(tests/rerank_oracle.py) that they contain what they claim, the GPU tests feed them to poi_rerank_lists / poi_score_lists.

A ragged fixture has one list per row: row r has the length LENGTHS[(r + shift) % len(LENGTHS)] and its scores follow the pattern
select_cases.PATTERNS[r % 10] (plateau, eight, eight_signed, special, dead, sparse, ...: ties, both zeros, NaN and the infinities sit in
the lists).  Ids are drawn WITH repetition from a table of n_item POIs; a repeated id copies the score and the prior of its first
occurrence on every second row (a tie between duplicates of one id: the position decides), every third row carries padding (-1) in the
middle of its list.  Priors are small integers and the blend weights dyadic, so that blended keys tie between different ids."""
import functools

import numpy as np

from tests import rerank_oracle as RO
from tests import select_cases as SC

CHUNK = 256                                         # poi_score_lists_chunk(): checked against the library by the GPU tests
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 1023, 1024, 1025, 4096)
TOO_LONG = RO.LEN_MAX + 1                           # a rejected row
# (rows, n_item, first length): 1, 31, 32, 33, 70 and 300 rows; tables of 13, 1037 and 5000 POIs
SHAPES = {"one": (1, 13, 4), "short": (31, 13, 0), "tile": (32, 1037, 3), "odd": (33, 1037, 7), "big": (70, 5000, 0), "many": (300, 1037, 11)}
LONG_ROW = {"big": 23}                              # the row of a fixture that holds TOO_LONG entries
# one list for all rows: (rows, n_item, entries)
SHARED = {"s_one": (1, 13, 1), "s_small": (33, 13, 65), "s_chunk": (70, 1037, CHUNK + 1), "s_max": (32, 5000, 4096)}
KS = (1, 20, 64, 65, 1000, 4096)
WEIGHTS = (0.5, 0.25)                               # dyadic: the blend of small integers is exact, so keys tie


def id_list(L, n_item, rng, r):
    """L ids of [0, n_item) with repetitions (about a fifth of the entries repeat an earlier one), padding in the middle on every third row."""
    ids = rng.integers(0, n_item, L).astype(np.int32)
    first = np.arange(L)
    if L >= 2:
        dup = np.nonzero(rng.random(L) < 0.2)[0]
        dup = dup[dup > 0]
        src = (rng.random(len(dup)) * dup).astype(np.int64)      # an earlier position
        for d, s in zip(dup, src):                  # (in ascending order: first[s] is already the first occurrence)
            ids[d] = ids[s]; first[d] = first[s]
    if r % 3 == 1 and L >= 3:
        hole = rng.choice(np.arange(1, L - 1), max(1, (L - 2) // 7), replace=False)
        ids[hole] = -1
    return ids, first


def list_row(L, n_item, r, rng):
    """(ids, scores, priors) of one list."""
    ids, first = id_list(L, n_item, rng, r)
    sc = SC.pattern_row(SC.pattern_of(r), max(L, 1), rng)[:L]
    pr = rng.integers(-2, 3, L).astype(np.float32)
    if r % 7 == 3 and L:
        pr[rng.integers(0, L)] = np.nan             # a NaN prior: that entry leaves under a blend only
    if r % 2 == 0:
        sc, pr = sc[first].copy(), pr[first].copy()
    return ids, sc, pr


@functools.lru_cache(maxsize=None)
def fixture(shape):
    """dict(n, n_item, off, cand, score, prior, bad): a ragged fixture.  bad = the rows poi_rerank_lists rejects."""
    n, N, shift = SHAPES[shape]
    rng = np.random.default_rng(2000 + 31 * n + N)
    rows = []
    for r in range(n):
        L = TOO_LONG if LONG_ROW.get(shape) == r else LENGTHS[(r + shift) % len(LENGTHS)]
        rows.append(list_row(L, N, r, rng))
    off, cand = RO.csr([x[0] for x in rows])
    cat = lambda i: np.concatenate([x[i] for x in rows]).astype(np.float32) if off[-1] else np.zeros(0, np.float32)
    return dict(name=shape, n=n, n_item=N, off=off, cand=cand, score=cat(1), prior=cat(2), bad=int(shape in LONG_ROW))


@functools.lru_cache(maxsize=None)
def shared_fixture(shape):
    """dict(n, n_item, off None, cand (C), score (n, C), prior (n, C), bad 0): one list for every row."""
    n, N, C = SHARED[shape]
    rng = np.random.default_rng(3000 + 31 * n + C)
    ids, first = id_list(C, N, rng, 1)
    sc = np.stack([SC.pattern_row(SC.pattern_of(r), C, rng) for r in range(n)])
    pr = rng.integers(-2, 3, (n, C)).astype(np.float32)
    even = np.arange(n) % 2 == 0
    sc[even] = sc[even][:, first]; pr[even] = pr[even][:, first]
    return dict(name=shape, n=n, n_item=N, off=None, cand=ids, score=sc, prior=pr, bad=0)


def any_fixture(shape):
    return shared_fixture(shape) if shape in SHARED else fixture(shape)


@functools.lru_cache(maxsize=None)
def expected(shape, with_prior):
    """The oracle's lists of a fixture at k = 4096: (ids, keys, positions, counts, bad rows).  The result is sorted best first, so the
    list of a smaller k is its first k columns."""
    F = any_fixture(shape)
    return RO.rerank(F["off"], F["cand"], F["n"], F["score"], RO.K_MAX, F["prior"] if with_prior else None, WEIGHTS)


def lengths(F):
    return np.diff(F["off"]) if F["off"] is not None else np.full(F["n"], len(F["cand"]))


def scoring_lists(n, n_item, seed, longest=1025):
    """Ragged id lists for poi_score_lists over a model of n rows: the LENGTHS up to `longest`, duplicates and padding as above."""
    rng = np.random.default_rng(seed)
    ls = [L for L in LENGTHS if L <= longest]
    return RO.csr([id_list(ls[(r + seed) % len(ls)], n_item, rng, r)[0] for r in range(n)])
