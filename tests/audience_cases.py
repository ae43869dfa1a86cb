"""The problems of tests/test_gpu_audience.py, built on the host: make_case of tests/test_gpu_near.py with 1037 users (32 full 32-row
tiles and one of 13 rows), 300 POIs and 70 query POIs (blocks of 32 / 32 / 6), the float64 oracle scores of every (POI, user) pair and
the train-visitor lists.  tests/test_audience_cpu.py checks on the CPU that the oracle alone separates every case.  No GPU import."""
import functools

import numpy as np

from tests import audience_oracle as AO
from tests.half_cases import half
from tests.test_gpu_near import last_of, make_case
from tests.test_gpu_session import seqs_of

K = 20
N_USER, N_ITEM, N_QUERY = 1037, 300, 70
NO_LAST = (3, 11, 40, 77, 1036)                      # spatial: rows without a last POI (no distance term); 1036 is the last row
# dim 4: the ragged last fragment of load_frag; 20: a dim that is no multiple of 8; 128 / 256: the single-buffer templates
RANK_CASES = [("bpr", 4), ("bpr", 20), ("bpr", 128), ("bpr", 256), ("gru", 20), ("spatial", 32), ("spatial", 128), ("vbpr", 20), ("fpmc", 20),
              ("fpmc", 128)]
HALF_CASES = [("bpr", 20), ("spatial", 128)]


def queries(seed, n_q=N_QUERY, n_item=N_ITEM):
    """n_q distinct query POIs in a random order."""
    return np.random.default_rng(seed).choice(n_item, n_q, replace=False).astype(np.int64)


def case_last(C):
    """The rows' last POI as the model scores with it: the last train POI, -1 for NO_LAST on the spatial case."""
    last = last_of(C["T"]).astype(np.int64)
    if C["kind"] == "spatial":
        last[[r for r in NO_LAST if r < len(last)]] = -1
    return last


def _case(kind, dim, seed, n_user, table_dtype="f32", twin_users=None):
    assert twin_users is None or kind != "spatial", "a spatial twin would need the same last POI: use bpr / gru"
    C = make_case(kind, dim, seed, n_user=n_user, n_item=N_ITEM, table_dtype=table_dtype)
    if twin_users is not None:                       # user row b a copy of row a (before `build` reads the table)
        a, b = twin_users
        C["users"][b] = C["users"][a]
        if C["term"] is not None:
            C["term"][1][b] = C["term"][1][a]
    T = C["T"]
    last = case_last(C)
    items = half(C["items"]) if table_dtype == "f16" else C["items"]
    pois = queries(seed + 1)
    return dict(C=C, last=last, pois=pois, sct=AO.scores_t(C["users"], items, last, C["term"], T),
                vis=AO.visitor_lists(seqs_of(T), N_ITEM, pois))


@functools.lru_cache(maxsize=None)
def rank_case(kind, dim, n_user=N_USER):
    """dict(C (make_case), last, pois (70 queries), sct ((n_item, n_user) float64 oracle scores), vis (CSR of the queries' train visitors))."""
    return _case(kind, dim, 500 + dim, n_user)


@functools.lru_cache(maxsize=None)
def half_case(kind, dim):
    """rank_case on a half POI table (the rule of tests/half_cases.py): the model is built with table_dtype="f16" from the unrounded
    float32 init, the oracle reads the rounded table.  sct32: the scores from the unrounded one."""
    R = _case(kind, dim, 900 + dim, N_USER, table_dtype="f16")
    C = R["C"]
    R["sct32"] = AO.scores_t(C["users"], C["items"], R["last"], C["term"], C["T"])
    return R


@functools.lru_cache(maxsize=None)
def twin_case(kind, a, b):
    """rank_case(kind, 20) with user row b a copy of row a: bitwise equal scores for every POI, the lower id first."""
    return _case(kind, 20, 520, N_USER, twin_users=(a, b))


def fixtures():
    """(name, query scores (n_q, n), candidate mask) of every ranking fixture, train visitors excluded."""
    for kind, dim in RANK_CASES:
        R = rank_case(kind, dim)
        yield "%s dim %d" % (kind, dim), R["sct"][R["pois"]], AO.candidate_mask(N_QUERY, N_USER, *R["vis"])
    for kind, dim in HALF_CASES:
        R = half_case(kind, dim)
        yield "%s dim %d f16" % (kind, dim), R["sct"][R["pois"]], AO.candidate_mask(N_QUERY, N_USER, *R["vis"])
