"""CPU tests of the fixtures of tests/test_gpu_half_serving.py (tests/half_cases.py): the oracle alone must separate every case on the
half-rounded table - clear top-(k + 1) gaps on at least 90 % of the rows (near, session recommend) and of the groups (the rule of
tests/test_group_cpu.py), clear decisions on at least route_cases.CLEAR_MIN of the route slots - and the half rounding must MATTER: on
every case the oracle from the unrounded float32 table differs from the oracle on the rounded one by more than the margin the GPU test
compares within, so that a kernel that served the float32 values (or the live table's) could not pass.  No GPU."""
import numpy as np
import pytest

from tests import group_oracle as GO
from tests import half_cases as HC
from tests import near_oracle as NO
from tests import route_cases as RC
from tests import route_oracle as RO
from tests.gpu_util import RTOL
from tests.test_gpu_session import oracle_rows, oracle_scores, seqs_of
from tests.test_gpu_near import last_of


def test_half_rounds_the_table_alone():
    P = HC.session_case("plain64")["P"]
    Ph = HC.rounded(P)
    assert sorted(Ph) == sorted(P) and all(np.array_equal(Ph[k], P[k]) for k in P if k != "lt")
    assert np.array_equal(Ph["lt"], np.float64(np.float16(np.float32(P["lt"])))) and np.abs(Ph["lt"] - P["lt"]).max() > 1e-5
    assert np.abs(Ph["lt"] - P["lt"]).max() <= 2.0 ** -12 * 0.5 * 1.0001            # half an ulp of a half below 0.5


# ---- sessions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.SESSION_CASES))
def test_session_states_move_under_the_rounding(name):
    C = HC.session_case(name)
    T = C["T"]
    assert T["n_user"] == 24 and T["n_item"] == 50 and T["lens"].min() >= 4 and T["lens"].max() == 12
    h32, s32 = oracle_rows(C["P"], T, seqs_of(T), spatial=C["spatial"])
    dh = np.abs(h32 - C["hts"]).max() / np.abs(C["hts"]).max()
    print("%s: the float32 table's states are %.1e off (bar %.0e)" % (name, dh, RTOL))
    assert dh > 10 * RTOL
    if C["spatial"]:
        assert np.abs(s32 - C["sts"]).max() / C["sts"].max() > RTOL


@pytest.mark.parametrize("name", HC.ADVANCE_CASES)
def test_advance_cases_move_under_the_rounding(name):
    A = HC.advance_case(name)
    C = A["C"]
    T = C["T"]
    h32, _ = oracle_rows(C["P"], T, [list(q) + [e] for q, e in zip(seqs_of(T), A["ev"])], spatial=C["spatial"])
    assert np.abs(h32 - A["h1"]).max() / np.abs(A["h1"]).max() > 10 * RTOL


@pytest.mark.parametrize("name", list(HC.RECOMMEND_CASES))
def test_recommend_cases_have_clear_gaps(name):
    C = HC.recommend_case(name)
    T = C["T"]
    mask = np.ones_like(C["sc"], bool)
    for k in HC.RECOMMEND_K:
        ok = NO.qualifying(C["sc"], mask, k)
        print("recommend %s k %d: %.0f %% of %d rows qualify" % (name, k, 100 * ok.mean(), len(ok)))
        assert ok.mean() >= 0.9, "recommend %s k %d: only %.1f %% of the rows have clear gaps: pick another seed" % (name, k, 100 * ok.mean())
    h32, s32 = oracle_rows(C["P"], T, seqs_of(T), spatial=C["spatial"])
    sc32 = oracle_scores(C["P"], T, h32, s32, last_of(T))
    assert np.abs(sc32 - C["sc"]).max(axis=1).max() > HC.score_margin(C["sc"])
    assert (NO.topk(sc32, mask, 20)[0] != NO.topk(C["sc"], mask, 20)[0]).any(), "the rounding changes no list"


# ---- near ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", HC.RANK_CASES)
def test_near_cases_have_clear_gaps(kind, dim):
    R = HC.near_case(kind, dim)
    assert R["sc"].shape == (HC.NEAR_USERS, HC.N_ITEM)
    for r_km, mask in R["masks"].items():
        ok = NO.qualifying(R["sc"], mask, HC.K)
        cnt = mask.sum(axis=1)
        print("near %s dim %d, %s km: %.0f %% of %d rows qualify, candidates %d..%d" % (kind, dim, r_km, 100 * ok.mean(), len(ok), cnt.min(), cnt.max()))
        assert ok.mean() >= 0.9, "near %s dim %d: only %.1f %% of the rows have clear gaps: pick another seed" % (kind, dim, 100 * ok.mean())
        assert cnt[3] == 0 and (cnt > HC.K).any()
    assert (R["masks"][5.0].sum(axis=1) < R["masks"][None].sum(axis=1)).any(), "the radius removes nothing"
    # the rounding matters: on some row a score of the float32 table is off by more than the margin a returned score is held within
    moved = np.abs(R["sc32"] - R["sc"]).max(axis=1)
    print("near %s dim %d: the float32 table's scores are up to %.1e off (margin %.1e)" % (kind, dim, moved.max(), HC.score_margin(R["sc"])))
    assert moved.max() > HC.score_margin(R["sc"])


# ---- group ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", GO.AGGS)
def test_group_fixtures_have_clear_gaps(agg):
    for name, sc, sc32, off, ids, eo, ei in HC.group_fixtures():
        assert sc.shape == (HC.GROUP_USERS, HC.N_ITEM)
        a, mask = GO.aggregate(sc, off, ids, agg), GO.candidate_mask(off, sc.shape[1], eo, ei)
        ok = GO.qualifying(a, mask, HC.K)
        print("group %s %s: %.0f %% of %d groups qualify" % (name, agg, 100 * ok.mean(), len(ok)))
        assert ok.mean() >= 0.9, "%s %s: only %.1f %% of the groups have clear gaps: pick another seed" % (name, agg, 100 * ok.mean())
        assert np.abs(GO.aggregate(sc32, off, ids, agg) - a).max() > HC.score_margin(a), "%s %s: the rounding moves no aggregate" % (name, agg)


def test_session_group_case_has_clear_gaps():
    S = HC.session_group_case()
    C = S["C"]
    T = C["T"]
    assert S["n_slot"] == T["n_user"] + 2

    def member_scores(P):                                # (the two slots without a check-in: h = 0)
        h, _ = oracle_rows(P, T, S["seqs"], spatial=False)
        return GO.member_scores(np.concatenate((h, np.zeros((2, h.shape[1])))), P["lt"])
    sc, sc32 = member_scores(C["Ph"]), member_scores(C["P"])
    mask = GO.candidate_mask(S["off"], T["n_item"], *S["ex"])
    for agg in GO.AGGS:
        a = GO.aggregate(sc, S["off"], S["ids"], agg)
        assert GO.qualifying(a, mask, HC.K).mean() >= 0.9
        assert np.abs(GO.aggregate(sc32, S["off"], S["ids"], agg) - a).max() > HC.score_margin(a)


# ---- routes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", HC.ROUTE_CASES)
def test_route_fixtures_have_clear_decisions(kind, name):
    C = HC.route_case(kind, name)
    share = float(C["clear"].mean())
    print("half route %s %s: %.0f %% of %d slots are clear, max|score| %.2f" % (kind, name, 100 * share, len(C["clear"]), C["max_abs"]))
    assert share >= RC.CLEAR_MIN, "%s %s: only %.1f %% of the slots are clear: pick another seed or shape" % (kind, name, 100 * share)
    # the rounding matters: the float32 table gives the oracle's best route of some slot another log-probability than the bar allows
    sc32 = RO.Scorer(kind, C["P"], C["T"])
    tol = 2 * C["steps"] * RTOL * max(1.0, C["max_abs"])
    worst = 0.0
    for u in range(min(len(C["hist"]), 8)):
        if C["paths"][u, 0, -1] >= 0:
            worst = max(worst, abs(RO.path_logp(sc32, C["hist"][u], C["paths"][u, 0])[0] - C["total"][u, 0]))
    print("half route %s %s: the float32 table's totals are up to %.1e off (bar %.1e)" % (kind, name, worst, tol))
    assert worst > tol
    if (kind, name) == HC.TILE_ADVANCE:
        assert len(C["hist"]) * C["beam"] >= 512, "the advance of the hypothesis rows must reach the session tile path"


# ---- AUC -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", HC.AUC_CASES)
def test_auc_cases_are_decided_and_the_planted_pairs_flip(kind, dim):
    A = HC.auc_case(kind, dim)
    sure = np.abs(A["margin"]) >= 1e-6 * A["scale"]
    assert sure.mean() >= 0.9
    pl = A["planted"]
    assert len(pl) == HC.AUC_PLANTED and sure[pl].all()
    assert ((A["margin"][pl] > 0) != (A["margin32"][pl] > 0)).all(), "a planted pair must change sign under the rounding"
    assert (A["tp"] < HC.N_ITEM).all() and (A["tq"] < HC.N_ITEM).all() and (A["margin"] > 0).any() and (A["margin"] < 0).any()


def test_hygiene_case_is_one_table_in_two_storage_forms():
    H, F = HC.hygiene_case()
    assert np.array_equal(H["C"]["items"], F["items"]) and np.array_equal(H["C"]["users"], F["users"])
    sc = NO.scores(F["users"], F["items"])
    assert NO.qualifying(sc, np.ones_like(sc, bool), HC.K).mean() >= 0.9
    sub = NO.scores(F["users"], F["items"][:HC.HYGIENE_SUB + 1])
    assert 4 * (HC.HYGIENE_SUB + 1) <= 2 * (HC.N_ITEM + 1) and NO.qualifying(sub, np.ones_like(sub, bool), HC.K).mean() >= 0.9


# ---- the families outside this file refuse a half table before they touch a device ------------------------------------------------------
def test_the_other_families_refuse_half_tables():
    import inspect
    from poi_amd import models as M
    for cls in (M.OboCARNN, M.OboFpmc_lr, M.OboPrme, M.OboPRPRM, M.OboPoi2vec, M.OboGeoIE, M.OboVBpr):
        n_pos = sum(p.default is inspect.Parameter.empty for p in list(inspect.signature(cls.__init__).parameters.values())[1:])
        with pytest.raises(TypeError, match="table_dtype"):
            cls(*[None] * n_pos, table_dtype="f16")
    for cls in (M.Lstm, M.Rnn):
        with pytest.raises(ValueError, match="float32 tables only"):
            cls(None, None, [0.01, 0.001], 4, 9, 8, 8, table_dtype="f16")
    for cls in (M.OboGru, M.OboSpatialGru, M.OboBpr):    # ... and the three that store one take the keyword
        assert "table_dtype" in inspect.signature(cls.__mro__[1].__init__).parameters or "table_dtype" in inspect.signature(cls.__init__).parameters
