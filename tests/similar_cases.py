"""The problems of tests/test_gpu_similar.py, built on the host: make_case of tests/test_gpu_near.py with 300 POIs (9 full 32-row tiles
and one of 12 rows), 70 query rows (blocks of 32 / 32 / 6) and 1037 users for the user side; the float64 oracle similarity of every
pair (tests/similar_oracle.py) and per-query exclusion lists.  tests/test_similar_cpu.py checks on the CPU that the oracle alone
separates every case.  No GPU import."""
import functools

import numpy as np

from tests import similar_oracle as SO
from tests.half_cases import half
from tests.test_gpu_near import make_case
from tests.test_gpu_session import seqs_of

K = 20
N_USER, N_ITEM, N_QUERY = 1037, 300, 70
# dim 4: the ragged last fragment of load_frag; 20: a dim that is no multiple of 8; 64: the double-buffered template's upper end;
# 128 / 256: the single-buffer templates
RANK_CASES = [("bpr", 4), ("bpr", 20), ("bpr", 128), ("bpr", 256), ("gru", 64), ("spatial", 128)]
HALF_CASES = [("bpr", 20), ("spatial", 128)]
GEO = [(0.0, 1.0), (0.5, 5.0), (0.5, 1.0)]           # (geo_weight, scale_km); with g = 0 the scale is not read
USER_CASES = [("bpr", 20), ("gru", 64), ("spatial", 128)]


def queries(seed, n_q, n):
    """n_q distinct query rows in a random order."""
    return np.random.default_rng(seed).choice(n, n_q, replace=False).astype(np.int64)


def lists(seed, qs, n):
    """One ascending exclusion list per query: up to 40 rows, every fourth empty; query 3 names itself among others, query 5 only itself."""
    rng = np.random.default_rng(seed)
    out = [np.sort(rng.choice(n, min(int(rng.integers(1, 40)), n), replace=False)) if i % 4 else np.zeros(0, np.int64) for i in range(len(qs))]
    if len(out) > 5:
        out[3] = np.unique(np.concatenate((out[3], [qs[3]])))
        out[5] = np.array([qs[5]], np.int64)
    return SO.csr(out)


def _case(kind, dim, seed, n_user, n_item=N_ITEM, table_dtype="f32", twins=None, zero=None):
    C = make_case(kind, dim, seed, n_user=n_user, n_item=n_item, table_dtype=table_dtype, twins=twins)
    if zero is not None:                             # (before `build` reads the table)
        C["items"][zero] = 0.0
    items = half(C["items"]) if table_dtype == "f16" else C["items"]
    n_q = min(N_QUERY, n_item)
    pois = queries(seed + 1, n_q, n_item)
    return dict(C=C, items=items[:n_item], coords=np.asarray(C["T"]["coords"], np.float64), pois=pois, ex=lists(seed + 2, pois, n_item))


@functools.lru_cache(maxsize=None)
def poi_case(kind, dim, n_item=N_ITEM):
    """dict(C (make_case, 70 users), items ((n_item, dim) float64 view of the float32 table), coords, pois (70 queries), ex (CSR))."""
    return _case(kind, dim, 1300 + dim, 70, n_item)


@functools.lru_cache(maxsize=None)
def half_case(kind, dim):
    """poi_case on a half POI table: the model is built with table_dtype="f16" from the unrounded float32 init, the oracle reads the
    rounded table."""
    return _case(kind, dim, 1700 + dim, 70, table_dtype="f16")


@functools.lru_cache(maxsize=None)
def twin_case(a, b):
    """poi_case("bpr", 20) with item row b a copy of row a, and their coordinates too: bitwise equal similarities to every third row."""
    R = _case("bpr", 20, 1320, 70, twins=(a, b))
    R["coords"] = R["coords"].copy(); R["coords"][b] = R["coords"][a]
    R["C"]["T"]["coords"] = R["coords"]
    return R


@functools.lru_cache(maxsize=None)
def zero_case(z):
    """poi_case("bpr", 20) with item row z all zero."""
    return _case("bpr", 20, 1321, 70, zero=z)


@functools.lru_cache(maxsize=None)
def sim_of(kind, dim, g, scale_km, which="poi"):
    """(n_item, n_item) float64 oracle similarity of a POI case."""
    R = {"poi": poi_case, "half": half_case}[which](kind, dim)
    return SO.sim_matrix(R["items"], R["coords"], g, scale_km)


@functools.lru_cache(maxsize=None)
def user_case(kind, dim):
    """dict(C (make_case, 1037 users), users (float64 view of the float32 rows), qs (70 query users), ex, sim ((n_user, n_user)))."""
    C = make_case(kind, dim, 1500 + dim, n_user=N_USER, n_item=N_ITEM)
    qs = queries(1501 + dim, N_QUERY, N_USER)
    return dict(C=C, users=C["users"], qs=qs, ex=lists(1502 + dim, qs, N_USER), sim=SO.sim_matrix(C["users"]))


@functools.lru_cache(maxsize=None)
def nearest_case(kind, dim):
    """Lists of 20 POIs for 70 rows (some -1 entries, row 7 all -1) and two history sets: "train" (the rows' train sequences) and a CSR
    with duplicates (row 2: its first POI again at the end), empty histories (rows 4 and 69) and a single-POI history (row 9)."""
    R = poi_case(kind, dim)
    T = R["C"]["T"]
    rng = np.random.default_rng(77 + dim)
    n = T["n_user"]
    lst = np.stack([rng.choice(N_ITEM, K, replace=False) for _ in range(n)]).astype(np.int64)
    lst[rng.random(lst.shape) < 0.05] = -1
    lst[7] = -1
    train = [np.asarray(s, np.int64) for s in seqs_of(T)]
    own = [rng.choice(N_ITEM, rng.integers(2, 12)) for _ in range(n)]
    own[2] = np.concatenate((own[2], own[2][:1]))
    own[4] = np.zeros(0, np.int64); own[n - 1] = np.zeros(0, np.int64)
    own[9] = own[9][:1]
    return dict(R=R, lists=lst, train=SO.csr(train), own=SO.csr(own))


def fixtures():
    """(name, query similarities (n_q, n), candidate mask) of every ranking fixture, with and without the exclusion lists."""
    for kind, dim in RANK_CASES:
        R = poi_case(kind, dim)
        for g, s in GEO:
            osc = sim_of(kind, dim, g, s)[R["pois"]]
            yield "%s dim %d g %g scale %g" % (kind, dim, g, s), osc, SO.candidate_mask(R["pois"], N_ITEM)
            yield "%s dim %d g %g scale %g, lists" % (kind, dim, g, s), osc, SO.candidate_mask(R["pois"], N_ITEM, *R["ex"])
    for kind, dim in HALF_CASES:
        R = half_case(kind, dim)
        for g, s in GEO:
            yield "%s dim %d f16 g %g scale %g" % (kind, dim, g, s), sim_of(kind, dim, g, s, "half")[R["pois"]], SO.candidate_mask(R["pois"], N_ITEM, *R["ex"])
    for kind, dim in USER_CASES:
        R = user_case(kind, dim)
        yield "users %s dim %d" % (kind, dim), R["sim"][R["qs"]], SO.candidate_mask(R["qs"], N_USER)
        yield "users %s dim %d, lists" % (kind, dim), R["sim"][R["qs"]], SO.candidate_mask(R["qs"], N_USER, *R["ex"])
