"""The problems of tests/test_gpu_diverse.py, built on the host: tests/test_diverse_cpu.py checks on the CPU that the oracle alone
separates them (clear score gaps for the pool, clear objective gaps for the re-ranking), the GPU tests build the models from them.
Cases come from make_case of tests/test_gpu_near.py, as tests/group_cases.py builds its own."""
import functools

import numpy as np

from tests import diverse_oracle as DO
from tests import near_oracle as NO
from tests.group_oracle import csr
from tests.test_gpu_near import last_of, make_case

K = 20
POOLS = (20, 33, 64)
N_USER, N_ITEM = 70, 3000                            # 70 rows: the 32-row tile boundary is crossed twice
NO_LAST = (3, 11, 40, 69)                            # spatial: rows without a last POI (no distance term)
SCALE_KM = 2.0
GAP = 1e-9                                           # the objective margin a float64 kernel is held to (tests/test_diverse_cpu.py)
# kind, dim: FPMC-LR scores at kdim = 2 dim, so its dim 256 (kdim 512) is beyond the kernels' dim <= 256
RANK_CASES = [(kind, dim) for kind in ("bpr", "spatial", "fpmc") for dim in (20, 64, 128, 256) if (kind, dim) != ("fpmc", 256)]
# (trade, geo_weight) of the end-to-end runs: the default, a mixed similarity, the embedding alone
E2E = ((0.7, 1.0), (0.3, 0.5), (0.7, 0.0))


def exclusion_lists(seed, n, n_item):
    """One ascending list per row: some empty, some long."""
    rng = np.random.default_rng(seed + 1)
    return csr([np.sort(rng.choice(n_item, rng.integers(1, min(200, n_item)), replace=False)) if r % 3 else np.zeros(0, np.int64) for r in range(n)])


def case_scores(C, last):
    T = C["T"]
    if C["term"] is None:
        return NO.scores(C["users"], C["items"])
    return NO.scores(C["users"], C["items"], last, C["term"][0], C["term"][1], T["coords"], T["dd_m"], T["n_dist"])


def mask_of(n, n_item, ex=(None, None)):
    mask = np.ones((n, n_item), bool)
    if ex[0] is not None:
        for r in range(n):
            mask[r, np.asarray(ex[1][ex[0][r]:ex[0][r + 1]], np.int64)] = False
    return mask


@functools.lru_cache(maxsize=None)
def rank_case(kind, dim):
    """dict(C (make_case), last (-1 for NO_LAST on the spatial case), sc (float64 oracle scores), ex, items, coords)."""
    C = make_case(kind, dim, 500 + dim, n_user=N_USER, n_item=N_ITEM)
    last = last_of(C["T"]).astype(np.int64)
    if kind == "spatial":
        last[list(NO_LAST)] = -1
    return dict(C=C, last=last, sc=case_scores(C, last), ex=exclusion_lists(dim, N_USER, N_ITEM), items=C["items"], coords=C["T"]["coords"])


@functools.lru_cache(maxsize=None)
def half_case():
    """The plain GRU at dim 64 on a half item table (table_dtype="f16"): the oracle reads the table's float16 rounding."""
    from tests.test_gpu_session import geo_problem, gru_init, plain_model
    T = geo_problem(571, n_user=N_USER, n_item=N_ITEM, n_dist=11, dim=64, len_min=4, len_max=8)
    P = gru_init(571, T)
    users = np.random.default_rng(572).uniform(-0.5, 0.5, (N_USER, 64)).astype(np.float32).astype(np.float64)
    items = P["lt"].astype(np.float16).astype(np.float64)

    def build(pa):
        m = plain_model(pa, T, P, table_dtype="f16")
        m.update_trained_users(users); m.set_coords(T["coords"])
        return m
    return dict(build=build, sc=NO.scores(users, items), items=items, coords=T["coords"], ex=exclusion_lists(64, N_USER, N_ITEM))


@functools.lru_cache(maxsize=None)
def wide_case():
    """BPR at dim 32 over 3000 POIs (94 item tiles: 64 slices leave most waves one tile or none) and 300 rows (above "diverse_split_max")."""
    C = make_case("bpr", 32, 541, n_user=300, n_item=N_ITEM)
    return dict(C=C, sc=NO.scores(C["users"], C["items"]), items=C["items"], coords=C["T"]["coords"], ex=exclusion_lists(32, 300, N_ITEM))


TWINS = ((57, 211), (5, 6), (100, 299))


@functools.lru_cache(maxsize=None)
def tie_case():
    """BPR at dim 32 over 300 POIs; every pair of TWINS shares its item row AND its coordinates: equal scores for every row, similarity
    1 to each other, equal similarity to every third POI."""
    from tests.test_gpu_session import geo_problem
    xy = geo_problem(523, n_user=N_USER, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)["coords"].copy()
    for a, b in TWINS:
        xy[b] = xy[a]
    C = make_case("bpr", 32, 523, n_user=N_USER, n_item=300, coords=xy)
    for a, b in TWINS:
        C["items"][b] = C["items"][a]
    return dict(C=C, sc=NO.scores(C["users"], C["items"]), items=C["items"], coords=xy)


@functools.lru_cache(maxsize=None)
def tiny_case(n_item):
    """BPR at dim 8 over a table shorter than k (5) or than the pool (13): m < k, m < pool."""
    from tests.gpu_util import toy_problem
    T = toy_problem(70 + n_item, n_user=6, n_item=n_item, dim=8, hot=min(8, n_item - 1))
    rng = np.random.default_rng(71 + n_item)
    u32 = lambda *sh: np.float64(np.float32(rng.uniform(-0.5, 0.5, sh)))
    users, items = u32(6, 8), u32(n_item + 1, 8)
    coords = np.stack((30.0 + rng.uniform(0, 0.05, n_item), 120.0 + rng.uniform(0, 0.05, n_item)), axis=1)
    ex = csr([[], [0, 2], [], list(range(n_item)), [1], []])
    return dict(T=T, users=users, items=items, coords=coords, sc=NO.scores(users, items), ex=ex)


POOL_M = (0, 1, 2, 20, 33, 63, 64)
POOL_ROWS = 3                                        # rows per pool size


@functools.lru_cache(maxsize=None)
def explicit_pools(dim):
    """Pools for the re-rank entry alone, 64 wide: POOL_ROWS rows of every size in POOL_M over the BPR case's tables at `dim` - distinct
    ids, float32 scores strictly descending, -1 / -inf behind the m entries.  A row's POIs come from the 90 nearest to a POI in the
    middle of the box (a few km across): at scale_km = 2 the far corners of the 40 km box have similarities of 1e-9, whose differences
    no margin of 1e-9 can separate under trade = 0.  dict(idx, score, items, coords, m)."""
    R = rank_case("bpr", dim)
    rng = np.random.default_rng(900 + dim)
    n = len(POOL_M) * POOL_ROWS
    idx, score = np.full((n, 64), -1, np.int64), np.full((n, 64), -np.inf)
    ms = np.repeat(POOL_M, POOL_ROWS)
    xy = R["coords"]
    central = np.nonzero((np.abs(xy[:, 0] - xy[:, 0].mean()) < 0.08) & (np.abs(xy[:, 1] - xy[:, 1].mean()) < 0.08))[0]
    for r, m in enumerate(ms):
        near = np.argsort(DO.dist_km(xy, np.arange(N_ITEM), rng.choice(central)), kind="stable")[:90]
        idx[r, :m] = rng.choice(near, m, replace=False)
        s = np.sort(rng.uniform(-3.0, 3.0, m))[::-1].astype(np.float32).astype(np.float64)
        assert m < 2 or np.diff(s).max() < 0.0
        score[r, :m] = s
    return dict(idx=idx, score=score, items=R["items"], coords=R["coords"], m=ms)


RERANK_GRID = [(k, trade, g) for k in (1, 20, 32) for trade in (0.0, 0.3, 0.7, 1.0) for g in (0.0, 0.5, 1.0)]


def rank_fixtures():
    """(name, scores, exclusion lists, item table, coords, planted) of every fixture the GPU tests pool and re-rank end to end."""
    for kind, dim in RANK_CASES:
        R = rank_case(kind, dim)
        yield "%s dim %d" % (kind, dim), R["sc"], (None, None), R["items"], R["coords"], False
        yield "%s dim %d, lists" % (kind, dim), R["sc"], R["ex"], R["items"], R["coords"], False
    H = half_case()
    yield "half", H["sc"], H["ex"], H["items"], H["coords"], False
    W = wide_case()
    yield "wide", W["sc"], (None, None), W["items"], W["coords"], False
    for n_item in (13, 5):
        Y = tiny_case(n_item)
        yield "tiny %d" % n_item, Y["sc"], Y["ex"], Y["items"], Y["coords"], False
    Tc = tie_case()
    yield "ties", Tc["sc"], (None, None), Tc["items"], Tc["coords"], True


def e2e_runs():
    """(fixture of rank_fixtures, pool, trade, geo_weight) of every end-to-end run: every fixture at pool 64 under each of E2E, and
    the smaller pools on one case."""
    for fx in rank_fixtures():
        for trade, g in E2E:
            yield fx, 64, trade, g
        if fx[0] == "bpr dim 128, lists":
            for pool in (20, 33):
                yield fx, pool, E2E[0][0], E2E[0][1]


def oracle_run(sc, ex, items, coords, k, pool, trade, geo_weight, scale_km=SCALE_KM):
    """The oracle end to end: (pool ids, pool scores (float32-rounded, as the kernel hands them on), counts, idx, pos, obj, min_gap)."""
    pi, ps, cnt = DO.pool(sc, mask_of(len(sc), sc.shape[1], ex), pool)
    ps = ps.astype(np.float32).astype(np.float64)
    return (pi, ps, cnt) + DO.rerank(pi, ps, items, coords, min(k, pool), trade, geo_weight, scale_km)
