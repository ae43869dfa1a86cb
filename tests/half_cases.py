"""The problems of tests/test_gpu_half_serving.py, built on the host: models whose POI table and evaluation snapshot are STORED as IEEE
half (table_dtype="f16", the storage form of BASELINE's config X) on the serving paths that read the table through a per-launch flag -
the session advance (session.hip), the restricted top-K (near.hip), group (group.hip) and route (route.hip) recommendation and the AUC
preference flags (misc.hip).  The rule is the one of diverse_cases.half_case(): the model is built with table_dtype="f16" from the
UNROUNDED float32 init, the oracle reads table.astype(float16).astype(float64).  The arithmetic stays float32 on converted rows, so the
bars are the existing ones: RTOL on states and values, exact lists on qualifying rows.  tests/test_half_cases_cpu.py checks on the CPU
that the oracle alone separates every case - and that the rounding moves every oracle result by more than the margin it is compared
within, so that a kernel serving the float32 init could not pass.  No GPU import here."""
import functools

import numpy as np

from tests import group_cases as GC
from tests import group_oracle as GO
from tests import near_oracle as NO
from tests import route_cases as RC
from tests import route_oracle as RO
from tests.gpu_util import RTOL
from tests.test_gpu_near import last_of, make_case, oracle_sc
from tests.test_gpu_session import geo_problem, gru_init, oracle_rows, oracle_scores, plain_model, seqs_of, spatial_init, spatial_model

K = 20


def half(a):
    """What a half table holds of a float32 table, as float64."""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def rounded(P):
    """The parameters the oracle runs from: only the POI table is stored as half."""
    return {**P, "lt": half(P["lt"])}


# ---- sessions: replay / advance on 24 users, 50 POIs, lengths 4 .. 12 ------------------------------------------------------------------
# name -> (kind, n_dist, dim); dim 20 is stored padded to kdim 64
SESSION_CASES = {"plain64": ("plain", 11, 64), "plain20": ("plain", 11, 20), "spatial128": ("spatial", 200, 128), "spatial256": ("spatial", 11, 256)}


def _session_problem(kind, n_dist, dim, seed, **shape):
    T = geo_problem(seed, n_dist=n_dist, dim=dim, **shape)
    spatial = kind == "spatial"
    P = spatial_init(dim, T) if spatial else gru_init(dim, T)

    def build(pa):
        return (spatial_model if spatial else plain_model)(pa, T, P, table_dtype="f16")
    return dict(kind=kind, spatial=spatial, T=T, P=P, Ph=rounded(P), build=build)


@functools.lru_cache(maxsize=None)
def session_case(name):
    """dict(kind, spatial, T, P (unrounded float32 init), Ph (lt rounded to half), build(pa) -> model, hts, sts (the oracle's states from
    Ph; sts None on the plain model))."""
    kind, n_dist, dim = SESSION_CASES[name]
    C = _session_problem(kind, n_dist, dim, 3 + dim + n_dist, n_user=24, n_item=50, len_min=4, len_max=12)
    C["hts"], C["sts"] = oracle_rows(C["Ph"], C["T"], seqs_of(C["T"]), spatial=C["spatial"])
    return C


ADVANCE_CASES = ("plain20", "spatial128")             # one batch through both advance kernels


@functools.lru_cache(maxsize=None)
def advance_case(name):
    """A session case with one further event for every slot: dict(C, ev, h1, s1 (the oracle's states after it; s1 None when plain))."""
    C = session_case(name)
    T = C["T"]
    ev = np.random.default_rng(51).integers(0, T["n_item"], T["n_user"])
    h1, s1 = oracle_rows(C["Ph"], T, [list(q) + [e] for q, e in zip(seqs_of(T), ev)], spatial=C["spatial"])
    return dict(C=C, ev=ev, h1=h1, s1=s1)


# Session.recommend: 64 slots over 300 POIs (the shapes of test_recommend_matches_the_oracle_ranks)
RECOMMEND_CASES = {"plain": ("plain", 11, 64), "spatial": ("spatial", 11, 128)}
RECOMMEND_K = (20, 40)                               # 40: beyond the fused kernels' k <= 32, through explicit score rows


@functools.lru_cache(maxsize=None)
def recommend_case(name):
    """session_case's dict over 300 POIs, and sc: the oracle's scores of every POI for every slot after the replay."""
    kind, n_dist, dim = RECOMMEND_CASES[name]
    C = _session_problem(kind, n_dist, dim, 160 + dim, n_user=64, n_item=300, len_min=4, len_max=8)
    T = C["T"]
    C["hts"], C["sts"] = oracle_rows(C["Ph"], T, seqs_of(T), spatial=C["spatial"])
    C["sc"] = oracle_scores(C["Ph"], T, C["hts"], C["sts"], last_of(T))
    return C


# ---- near / group: make_case over 300 POIs ---------------------------------------------------------------------------------------------
# dim 4 and dim 20: BPR keeps its native dim under f16 - the ragged last fragment of load_frag (k0 < D with D % 8 != 0); dim 256: the
# single-buffer template of the tile kernels; gru / spatial: the GRU family's snapshot
RANK_CASES = [("bpr", 4), ("bpr", 20), ("bpr", 256), ("gru", 64), ("spatial", 128)]
N_ITEM = 300
NEAR_USERS, GROUP_USERS = 70, 80
NEAR_RADII = (None, 5.0)


def row_lists(seed, n, n_item):
    """One ascending exclusion list per row: up to 40 ids, some empty; row 3 lists every POI."""
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(n_item, rng.integers(0, 40), replace=False)) if r % 4 else np.zeros(0, np.int64) for r in range(n)]
    lists[3] = np.arange(n_item)
    return GO.csr(lists)


def _half_view(C):
    """The case as the oracle of a half model sees it: the item table rounded."""
    return dict(C, items=half(C["items"]))


@functools.lru_cache(maxsize=None)
def near_case(kind, dim):
    """dict(C (make_case, table_dtype="f16"), anchor, sc (oracle scores from the rounded table), sc32 (from the unrounded one), ex,
    masks {within_km: candidate mask under ex})."""
    C = make_case(kind, dim, 700 + dim, n_user=NEAR_USERS, n_item=N_ITEM, table_dtype="f16")
    T = C["T"]
    anchor = last_of(T)
    ex = row_lists(dim, NEAR_USERS, N_ITEM)
    masks = {r_km: NO.candidate_mask(T["coords"], anchor, r_km, *ex) for r_km in NEAR_RADII}
    return dict(C=C, anchor=anchor, sc=oracle_sc(_half_view(C), anchor), sc32=oracle_sc(C, anchor), ex=ex, masks=masks)


@functools.lru_cache(maxsize=None)
def group_case(kind, dim):
    """group_cases.rank_case on a half table: dict(C, last, sc (member scores from the rounded table), sc32, off, ids, ex)."""
    C = make_case(kind, dim, 800 + dim, n_user=GROUP_USERS, n_item=N_ITEM, table_dtype="f16")
    T = C["T"]
    last = last_of(T).astype(np.int64)
    if kind == "spatial":
        last[list(GC.NO_LAST)] = -1

    def scores(items):
        if kind != "spatial":
            return GO.member_scores(C["users"], items)
        return GO.member_scores(C["users"], items, last, C["term"][0], C["term"][1], T["coords"], T["dd_m"], T["n_dist"])
    off, ids = GO.csr(GC.mixed_groups(dim, GROUP_USERS))
    return dict(C=C, last=last, sc=scores(half(C["items"])), sc32=scores(C["items"]), off=off, ids=ids,
                ex=GC.exclusion_lists(dim, len(off) - 1, N_ITEM))


def group_fixtures():
    """(name, member scores, their float32-table counterpart, off, ids, ex_off, ex) of every group fixture."""
    for kind, dim in RANK_CASES:
        R = group_case(kind, dim)
        yield "%s dim %d" % (kind, dim), R["sc"], R["sc32"], R["off"], R["ids"], None, None
        yield "%s dim %d, lists" % (kind, dim), R["sc"], R["sc32"], R["off"], R["ids"], R["ex"][0], R["ex"][1]


@functools.lru_cache(maxsize=None)
def session_group_case():
    """Session.recommend_group on the plain dim-64 case: three check-ins per slot, the last two slots never check in.
    dict(C, n_slot, seqs, off, ids, ex)."""
    C = recommend_case("plain")
    T = C["T"]
    rng = np.random.default_rng(13)
    n = T["n_user"]
    off, ids = GO.csr([rng.choice(n, s, replace=False) for s in (1, 3, 4, 4, 6, 17, 33, 40)] + [[n, 3, n + 1], [7, 7], []])
    return dict(C=C, n_slot=n + 2, seqs=[T["train"][0][u, :3] for u in range(n)], off=off, ids=ids, ex=GC.exclusion_lists(14, len(off) - 1, T["n_item"]))


# ---- routes: the fixtures of tests/route_cases.py, scored from the rounded table -------------------------------------------------------
ROUTE_CASES = [("plain", "d64"), ("spatial", "d128"), ("spatial", "d256"), ("spatial", "d20"), ("plain", "d16x144")]
TILE_ADVANCE = ("plain", "d16x144")                  # 576 hypothesis rows: the advance takes sess_tile_kernel


@functools.lru_cache(maxsize=None)
def route_case(kind, name):
    """route_cases.problem with P["lt"] rounded for the scorer, and route_cases.solve on it: dict(T, P (unrounded: what the model is
    built from), Ph, build(pa) -> model, kind, beam, steps, hist, scorer, paths, total, steplp, clear, max_abs)."""
    C = dict(RC.problem(kind, name))
    C["Ph"] = rounded(C["P"])
    C["build"] = lambda pa: (spatial_model if kind == "spatial" else plain_model)(pa, C["T"], C["P"], table_dtype="f16")
    sc = RO.Scorer(kind, C["Ph"], C["T"])
    res = [RO.beam_search(sc, h, C["beam"], C["steps"], exclude=(h[-1],)) for h in C["hist"]]
    C.update(scorer=sc, paths=np.array([r["paths"] for r in res]), total=np.array([r["total"] for r in res]),
             steplp=np.array([r["steplp"] for r in res]), clear=np.array([RO.clear(r["gaps"], sc.max_abs) for r in res]), max_abs=sc.max_abs)
    return C


# ---- AUC preference flags ---------------------------------------------------------------------------------------------------------------
AUC_CASES = [("bpr", 20), ("gru", 64)]
AUC_PLANTED = 8


def auc_margins(users, items, tp, tq):
    """float64 margins users[r] . (items[tp[r, e]] - items[tq[r, e]]) and max|score| over the table."""
    users, items = np.asarray(users, np.float64), np.asarray(items, np.float64)
    return np.einsum("nd,nld->nl", users, items[tp] - items[tq]), float(np.abs(users @ items[:-1].T).max())


@functools.lru_cache(maxsize=None)
def auc_case(kind, dim):
    """The near case's model with the test pair of AUC_PLANTED users replaced by one whose margin changes SIGN under the half rounding (and
    is clear on both tables): the flags of a kernel that read the float32 values would differ from the oracle's there.
    dict(C, tp, tq, margin (rounded table), margin32, scale, planted)."""
    C = make_case(kind, dim, 700 + dim, n_user=NEAR_USERS, n_item=N_ITEM, table_dtype="f16")
    T = C["T"]
    tp, tq = T["test"][0], T["test"][2]                 # (n_user, 1): the arrays the model is built from, changed in place below
    s16, s32 = C["users"] @ half(C["items"])[:-1].T, C["users"] @ C["items"][:-1].T
    lim = 1e-6 * np.abs(s16).max()
    planted = []
    for u in range(NEAR_USERS):
        m16, m32 = s16[u][:, None] - s16[u][None, :], s32[u][:, None] - s32[u][None, :]
        p, q = np.nonzero((m16 >= 4 * lim) & (m32 <= -4 * lim))
        if len(p) and len(planted) < AUC_PLANTED:
            tp[u, 0], tq[u, 0] = p[0], q[0]
            planted.append(u)
    margin, scale = auc_margins(C["users"], half(C["items"]), tp, tq)
    margin32, _ = auc_margins(C["users"], C["items"], tp, tq)
    return dict(C=C, tp=tp, tq=tq, margin=margin, margin32=margin32, scale=scale, planted=np.array(planted, np.int64))


# ---- registry hygiene: a float32 model of the shapes of a dropped half model ------------------------------------------------------------
HYGIENE_SUB = 149                                    # POIs of a float32 table that fits into the half snapshot's memory (300 + 1 rows)


@functools.lru_cache(maxsize=None)
def hygiene_case():
    """(half case, float32 case) of BPR at dim 20 from one seed: the same tables, stored as half and as float32."""
    return near_case("bpr", 20), make_case("bpr", 20, 720, n_user=NEAR_USERS, n_item=N_ITEM)


def score_margin(sc):
    """The margin `check` of tests/test_gpu_near.py holds a returned score within."""
    return RTOL * np.abs(sc).max()
