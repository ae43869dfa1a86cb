"""-m gpu tests of the group recommendation (poi_group_topk / poi_group_topk_scores -> models.recommend_group,
Session.recommend_group): ranking under both rules, tiny tables, one-member groups, least misery under permutations, launch regimes,
exclusions, the explicit-score entry, ties, sessions and the contract - against the float64 oracle of tests/group_oracle.py run from
the float32-rounded tables, with the `check` contract of tests/test_gpu_near.py.  The problems are those of tests/group_cases.py."""

import numpy as np
import pytest

from tests import group_cases as GC
from tests import group_oracle as GO
from tests import near_oracle as NO
from tests.test_gpu_near import AL, check, last_of

pytestmark = pytest.mark.gpu

K = GC.K
AGG_ID = {"mean": 0, "min": 1}


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def rec(m, off, ids, k=K, **kw):
    return m.recommend_group((off, ids), k, return_scores=True, return_counts=True, **kw)


def same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def build_rank_model(pa, R):
    """The case's model; on the spatial case the members of NO_LAST lose their last POI in the scoring snapshot."""
    m = R["C"]["build"](pa)
    if R["C"]["kind"] == "spatial":
        m._last_poi[list(GC.NO_LAST)] = -1
    return m


def oracle(sc, off, ids, agg, ex=(None, None)):
    return GO.aggregate(sc, off, ids, agg), GO.candidate_mask(off, sc.shape[1], ex[0], ex[1])


# ---- 1: ranking ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", GC.RANK_CASES)
def test_ranking_matches_the_oracle(pa, kind, dim):
    R = GC.rank_case(kind, dim)
    m = build_rank_model(pa, R)
    assert m.kdim == {"bpr": dim, "spatial": 64 if dim < 64 else dim, "fpmc": 2 * dim}[kind]
    off, ids = R["off"], R["ids"]
    assert sorted(set(np.diff(off).tolist())) == [0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 32, 33, 70]
    for agg in GO.AGGS:
        for name, ex in (("", (None, None)), (", lists", R["ex"])):
            a, mask = oracle(R["sc"], off, ids, agg, ex)
            idx, sc, cnt = check(rec(m, off, ids, agg=agg, exclude=None if ex[0] is None else ex), a, mask, K, "%s dim %d %s%s" % (kind, dim, agg, name))
            assert cnt[9] == 0 and np.all(idx[9] == -1)      # the empty group
    assert m.ctx.take_bad_ids() == 0


@pytest.mark.parametrize("n_item", [13, 5])
def test_tiny_tables(pa, n_item):
    Y = GC.tiny_case(n_item)
    T = Y["T"]
    m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=AL, n_user=T["n_user"], n_item=n_item, n_in=8, n_hidden=8,
                         init=dict(ux=Y["users"], lt=Y["items"]))
    m.update_trained_items(); m.update_trained_users()
    for agg in GO.AGGS:
        a, mask = oracle(Y["sc"], Y["off"], Y["ids"], agg, Y["ex"])
        idx, sc, cnt = check(rec(m, Y["off"], Y["ids"], agg=agg, exclude=Y["ex"]), a, mask, K, "tiny %d %s" % (n_item, agg))
        assert cnt.tolist() == [n_item, n_item - 2, n_item, 0, 0]
        assert np.all(idx[0, n_item:] == -1) and np.all(idx[0, :n_item] >= 0) and np.all(np.isneginf(sc[0, n_item:]))


# ---- 2: one-member groups are the single-user entries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128)])
def test_one_member_groups(pa, kind, dim):
    import torch
    R = GC.rank_case(kind, dim)
    C = R["C"]
    m = C["build"](pa)                                       # (every user keeps their last POI: the model's own entries are the reference)
    rows = np.arange(GC.N_USER)
    off = np.arange(GC.N_USER + 1)
    osc = R["sc"] if kind == "bpr" else GO.member_scores(C["users"], C["items"], last_of(C["T"]), C["term"][0], C["term"][1], C["T"]["coords"],
                                                         C["T"]["dd_m"], C["T"]["n_dist"])
    ok = NO.qualifying(osc, np.ones_like(osc, bool), K)
    assert ok.mean() >= 0.9
    top = m.compute_sub_topk(rows, K).cpu().numpy()
    for agg in GO.AGGS:
        idx, sc, cnt = rec(m, off, rows, agg=agg)
        assert np.array_equal(idx.cpu().numpy()[ok], top[ok]) and np.all(cnt.cpu().numpy() == GC.N_ITEM)
        for c0 in range(0, K, 8):                            # (compute_sub_target_rank takes up to 8 targets per row)
            w = min(8, K - c0)
            rank, s2 = m.compute_sub_target_rank(rows, targets=idx[:, c0:c0 + w].contiguous(), return_scores=True)
            assert torch.equal(s2, sc[:, c0:c0 + w]), "the scores differ from poi_score_rank's"
            assert np.array_equal(rank.cpu().numpy(), np.tile(np.arange(c0, c0 + w), (GC.N_USER, 1)))


# ---- 3: least misery is exact -------------------------------------------------------------------------------------------------------------
def test_least_misery_is_invariant_under_permutations(pa):
    R = GC.rank_case("spatial", 128)
    m = build_rank_model(pa, R)
    off, ids = R["off"], R["ids"]
    ref = rec(m, off, ids, agg="min", exclude=R["ex"])
    rng = np.random.default_rng(8)
    for _ in range(2):
        perm = np.concatenate([rng.permutation(ids[off[g]:off[g + 1]]) for g in range(len(off) - 1)])
        assert not np.array_equal(perm, ids)
        assert same(rec(m, off, perm, agg="min", exclude=R["ex"]), ref)


# ---- 4: launch regimes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(pa):
    W = GC.wide_case()
    return W, W["C"]["build"](pa)


@pytest.mark.parametrize("agg", GO.AGGS)
def test_both_regimes_and_every_split_give_the_same_bits(wide, agg):
    W, m = wide
    off, ids = W["off"], W["ids"]
    n_grp = len(off) - 1
    assert n_grp == 300
    default = 256
    keys = ("group_path", "group_splits", "group_split_max")
    try:
        ref = rec(m, off, ids, agg=agg)                      # 300 groups: above the switch point
        assert {k: m.ctx.last_plan(k) for k in keys} == dict(group_path=0, group_splits=0, group_split_max=default)
        check(ref, *oracle(W["sc"], off, ids, agg), K, "wide %s" % agg)
        assert same(rec(m, off, ids, agg=agg), ref), "two identical calls differ"
        for grid in (1, 2, 7, 64):
            m.ctx.set_option("group_split_max", 1 << 30); m.ctx.set_option("group_grid", grid)
            out = rec(m, off, ids, agg=agg)
            assert {k: m.ctx.last_plan(k) for k in keys} == dict(group_path=1, group_splits=grid, group_split_max=1 << 30)
            assert same(out, ref), "grid %d differs from the tile path" % grid
        m.ctx.set_option("group_split_max", default); m.ctx.set_option("group_grid", 0)
        # a group alone (the split path chooses its own slices) against the same group inside the call of 300
        for g in (0, 5, 7, 8, 9, 150, 299):
            alone = rec(m, np.array([0, off[g + 1] - off[g]]), ids[off[g]:off[g + 1]], agg=agg)
            plan = {k: m.ctx.last_plan(k) for k in keys}
            assert plan["group_path"] == 1 and 2 <= plan["group_splits"] <= 64, plan
            assert same(alone, tuple(t[g:g + 1] for t in ref)), "group %d alone differs" % g
        # ... and the first 19 groups as a call of their own, forced onto the tile path
        m.ctx.set_option("group_split_max", 0)
        sub = rec(m, off[:20], ids[:off[19]], agg=agg)
        assert m.ctx.last_plan("group_path") == 0 and same(sub, tuple(t[:19] for t in ref))
    finally:
        m.ctx.set_option("group_split_max", default); m.ctx.set_option("group_grid", 0)


# ---- 5: exclusions ----------------------------------------------------------------------------------------------------------------------------
def test_exclusions(pa):
    from poi_amd import data
    R = GC.rank_case("bpr", 20)
    T = R["C"]["T"]
    m = build_rank_model(pa, R)
    off, ids = R["off"], R["ids"]
    xo, xi = data.group_exclusion_csr(*data.train_exclusion_csr(T["off"], T["p_flat"], T["n_item"]), off, ids, T["n_item"])
    for g in range(len(off) - 1):
        assert set(xi[xo[g]:xo[g + 1]].tolist()) == {int(p) for u in ids[off[g]:off[g + 1]] for p in T["p_flat"][T["off"][u]:T["off"][u + 1]]}
    for agg in GO.AGGS:
        a, mask = oracle(R["sc"], off, ids, agg, (xo, xi))
        out = check(rec(m, off, ids, agg=agg, exclude="train"), a, mask, K, "exclude train %s" % agg)
        assert (out[2][np.diff(off) > 0] < T["n_item"]).all()
        got = rec(m, off, ids, agg=agg, exclude=(xo, xi))
        assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(out, got)), "exclude='train' differs from the explicit union lists"
    # every POI excluded: nothing is left
    n_grp = len(off) - 1
    idx, sc, cnt = (t.cpu().numpy() for t in rec(m, off, ids, exclude=(np.arange(n_grp + 1) * T["n_item"], np.tile(np.arange(T["n_item"]), n_grp))))
    assert np.all(cnt == 0) and np.all(idx == -1) and np.all(np.isneginf(sc))
    with pytest.raises(ValueError):
        m.recommend_group((off, ids), K, exclude="last")


# ---- 6: the entry on explicit score rows ----------------------------------------------------------------------------------------------------
def raw_scores(pa, m, scores, off, ids, agg, ex, k):
    import torch
    ptr = pa.models._ptr
    dev = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).to(m.device)
    s, o, i = dev(scores, np.float32), dev(off, np.int32), dev(ids, np.int32)
    eo, ei = (dev(ex[0], np.int32), dev(ex[1], np.int32)) if ex[0] is not None else (None, None)
    n_grp = len(off) - 1
    idx = torch.empty((n_grp, k), dtype=torch.int32, device=m.device)
    sc = torch.empty((n_grp, k), dtype=torch.float32, device=m.device)
    cnt = torch.empty(n_grp, dtype=torch.int32, device=m.device)
    m.ctx.check(m.lib.poi_group_topk_scores(m.ctx.handle, ptr(s), s.shape[0], s.shape[1], ptr(o), ptr(i), n_grp, AGG_ID[agg], ptr(eo), ptr(ei), k,
                                            ptr(idx), ptr(sc), ptr(cnt), m._stream()))
    return idx, sc, cnt


def test_scores_entry_gives_the_oracles_lists(pa):
    R = GC.rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    off, ids = R["off"], R["ids"]
    rows = np.float64(np.float32(R["sc"]))                   # the oracle's score rows, float32-rounded: what the kernel reads
    dyadic = np.random.default_rng(12).integers(-2048, 2048, rows.shape) / 1024.0      # sums of 70 such values are exact in float32
    for name, full in (("oracle rows", rows), ("dyadic rows", dyadic)):
        for agg in GO.AGGS:
            a, mask = oracle(full, off, ids, agg, R["ex"])
            # (the dyadic rows tie by construction - few distinct values - and are held to the exact lists below, ties included)
            idx, sc, cnt = check(raw_scores(pa, m, full, off, ids, agg, R["ex"], K), a, mask, K, "%s %s" % (name, agg),
                                 min_ok=0.9 if name == "oracle rows" else 0.0)
            if agg == "min" or name == "dyadic rows":        # nothing is rounded on the way to the comparison: every list, exactly
                assert np.array_equal(idx, GO.topk(a, mask, K)[0]), (name, agg)
            if agg == "min":
                assert np.array_equal(sc, np.float32(GO.topk(a, mask, K)[1]))
    assert m.ctx.take_bad_ids() == 0


def small_groups(seed, n_user):
    rng = np.random.default_rng(seed)
    return GO.csr([rng.choice(n_user, s, replace=False) for s in (1, 2, 3, 4, 4, 5, 7, min(n_user, 20))] + [[1, 1, 0], []])


def test_scores_route_through_prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(45, 700, 14, 4)
    m = _model(ds)
    m.update_trained_items()
    users = np.arange(ds.n_user)
    full = m.compute_sub_all_scores(users)
    full = np.float64(full.reshape(ds.n_user, -1, ds.n_item)[:, 0])       # row 0 of every user: the query is the last train POI
    off, ids = small_groups(21, ds.n_user)
    for agg in GO.AGGS:
        check(rec(m, off, ids, agg=agg), *oracle(full, off, ids, agg), K, "prme %s" % agg)


def test_scores_route_through_poi2vec(pa):
    """(user, position) score rows: a member's row is the one of their next position, position 0."""
    from poi_amd import data as D, harness
    ds = D.make_poi2vec_synthetic(60, 200, 12, 13, local=0.9, n_nbr=8)
    m = harness.poi2vec_model(ds, dict(latent_size=20, seed=5, softmax_axis="items", eval_context="test"))
    m.update_trained_params()
    users = np.arange(60)
    full = m.compute_sub_all_scores(users)
    full = np.float64(full.reshape(60, -1, m.n_item)[:, 0])
    off, ids = small_groups(23, 60)
    for agg in GO.AGGS:
        check(rec(m, off, ids, agg=agg), *oracle(full, off, ids, agg), K, "poi2vec %s" % agg)


def carnn_model(pa):
    from tests.gpu_util import toy_problem
    from tests.test_gpu_carnn import _model, _params
    T = toy_problem(540, n_user=21, n_item=150, n_dist=23, dim=32, len_max=9)
    rng = np.random.default_rng(9)
    coords = np.stack([40.0 + rng.random(150) * 0.05, -74.0 + rng.random(150) * 0.05], 1)
    m = _model(pa, T, _params(540, T), coords=coords)
    m.update_trained_items(); m.update_trained_dists()
    m.update_trained_users(m.predict(np.arange(21, dtype=np.int32)))
    return m


def test_scores_route_through_carnn_and_its_session_is_refused(pa):
    m = carnn_model(pa)
    full = np.float64(m.compute_sub_all_scores(np.arange(21)))
    off, ids = small_groups(22, 21)
    for agg in GO.AGGS:
        check(rec(m, off, ids, agg=agg), *oracle(full, off, ids, agg), K, "carnn %s" % agg)
    with pytest.raises(pa._lib.PoiError, match="OboCARNN"):
        m.cell_session().recommend_group([[0, 1]], K)


# ---- 7: ties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", GO.AGGS)
def test_planted_ties_come_out_in_ascending_id_order(pa, agg):
    Tc = GC.tie_case()
    m = Tc["C"]["build"](pa)
    lo, hi = Tc["twins"]
    off, ids = Tc["off"], Tc["ids"]
    n_grp, N = len(off) - 1, Tc["sc"].shape[1]
    keep = np.union1d(np.random.default_rng(5).choice(N, 28, replace=False), [lo, hi])
    gone = np.setdiff1d(np.arange(N), keep)                  # at most 30 candidates: both twins are on every list
    ex = (np.arange(n_grp + 1) * len(gone), np.tile(gone, n_grp))
    a, mask = oracle(Tc["sc"], off, ids, agg, ex)
    assert np.array_equal(a[:, lo], a[:, hi])
    idx, sc, cnt = (t.cpu().numpy() for t in rec(m, off, ids, 32, agg=agg, exclude=ex))
    assert np.array_equal(cnt, mask.sum(axis=1))
    for g in np.nonzero(np.diff(off) > 0)[0]:
        at = int(np.nonzero(idx[g] == lo)[0][0])
        assert idx[g, at + 1] == hi and sc[g, at] == sc[g, at + 1], g


# ---- 8: sessions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "lstm"])
def test_session_recommend_group(pa, kind):
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    if kind == "spatial":
        P = TS.spatial_init(32, T)
        s = TS.spatial_model(pa, T, P).session(n_slot=T["n_user"] + 2)
    else:
        P = TC.params("lstm", 60, T)
        s = TC.model(pa, "lstm", T, P).cell_session(n_slot=T["n_user"] + 2)
    for t in range(3):                                       # three check-ins per slot; the last two slots never check in
        s.advance(np.arange(T["n_user"]), T["train"][0][:, t])
    st = s.state()
    users = np.float64(np.float32(st["h"]))                  # the kernel reads the float32 rounding of the state
    if kind == "spatial":
        msc = GO.member_scores(users, P["lt"], st["last_poi"], P["wd"], np.float64(st["sts"]), T["coords"], T["dd_m"], T["n_dist"])
    else:
        msc = GO.member_scores(users, P["lt"])
    assert np.array_equal(st["last_poi"][-2:], [-1, -1]) and np.array_equal(st["last_poi"][:-2], T["train"][0][:, 2])
    rng = np.random.default_rng(13)
    off, ids = GO.csr([rng.choice(T["n_user"], n, replace=False) for n in (1, 3, 4, 4, 6, 17, 33, 40)] + [[64, 3, 65], [7, 7], []])
    ex = GC.exclusion_lists(14, len(off) - 1, T["n_item"])
    for agg in GO.AGGS:
        a, mask = oracle(msc, off, ids, agg, ex)
        out = s.recommend_group((off, ids), K, agg=agg, exclude=ex, return_scores=True, return_counts=True)
        check(out, a, mask, K, "session %s %s" % (kind, agg))
    plain = s.recommend_group([[5, 6], [64]], K)
    assert plain.shape == (2, K) and np.array_equal(plain[1].cpu().numpy(), np.arange(K))      # no check-in: 0 . items, ascending id
    with pytest.raises(IndexError):
        s.recommend_group([[0, T["n_user"] + 2]], K)
    with pytest.raises(ValueError):
        s.recommend_group([[0]], K, exclude="train")


# ---- 9: contract ----------------------------------------------------------------------------------------------------------------------------
def test_contract(pa):
    import torch
    R = GC.rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    off, ids = R["off"], R["ids"]
    n_grp = len(off) - 1
    dev = lambda v: torch.as_tensor(np.asarray(v, np.int32)).to(m.device)
    clean = tuple(t.cpu().numpy() for t in rec(m, off, ids, agg="min", exclude=R["ex"]))

    def one_bad(groups, exclude, g_bad):
        with pytest.raises(IndexError):
            m.recommend_group(groups, K, agg="min", exclude=exclude)
        idx, sc, cnt = (t.cpu().numpy() for t in m.recommend_group(groups, K, agg="min", exclude=exclude, return_scores=True, return_counts=True, sync=False))
        assert m.ctx.take_bad_ids() == 1
        assert np.all(idx[g_bad] == -1) and np.all(np.isneginf(sc[g_bad])) and cnt[g_bad] == 0
        good = np.arange(n_grp) != g_bad
        assert all(np.array_equal(x[good], y[good]) for x, y in zip((idx, sc, cnt), clean)), "the other groups changed"

    dex = tuple(dev(v) for v in R["ex"])
    for bad_value in (GC.N_USER, -1):                        # a member out of range: host lists are refused, a device list is the kernel's
        bad = ids.copy(); bad[off[6] + 5] = bad_value        # (group 6: 33 members)
        with pytest.raises(IndexError):
            m.recommend_group((off, bad), K, exclude=R["ex"])
        assert m.ctx.take_bad_ids() == 0
        one_bad((dev(off), dev(bad)), dex, 6)
    # a malformed exclusion list: ids not ascending / out of range (device lists)
    eo, ei = R["ex"]
    g_x = int(np.nonzero(np.diff(eo) >= 2)[0][0])
    for make in (lambda e: e.__setitem__(slice(eo[g_x], eo[g_x] + 2), e[eo[g_x]:eo[g_x] + 2][::-1].copy()), lambda e: e.__setitem__(eo[g_x + 1] - 1, GC.N_ITEM)):
        e2 = ei.copy(); make(e2)
        one_bad((off, ids), (dev(eo), dev(e2)), g_x)
    # descending offsets in a device CSR: group 1 is rejected, the groups around it are ranked
    o2 = np.array([0, 3, 2, 5])
    idx = m.recommend_group((dev(o2), dev(ids[:5])), K, sync=False).cpu().numpy()
    assert m.ctx.take_bad_ids() == 1 and np.all(idx[1] == -1) and idx[0, 0] >= 0 and idx[2, 0] >= 0
    with pytest.raises(ValueError):
        m.recommend_group((dev([0, 9]), dev(ids[:5])), K)      # offsets that leave the id list address memory: refused on the host
    # sizes
    with pytest.raises(pa._lib.PoiError, match="k <= 32"):
        m.recommend_group((off, ids), 33)
    with pytest.raises(ValueError):
        m.recommend_group((off, ids), K, agg="median")
    assert m.recommend_group([], K).shape == (0, K)
    u6 = torch.zeros((4, 6), dtype=torch.float32, device=m.device)
    out = torch.empty((1, K), dtype=torch.int32, device=m.device)
    ptr = pa.models._ptr
    for dim, k, agg in ((6, K, 0), (8, 33, 0), (8, K, 2)):
        rc = m.lib.poi_group_topk(m.ctx.handle, ptr(u6), ptr(m.trained_items.t), 4, GC.N_ITEM, dim, None, None, None, None, None, None, 0, 0.0,
                                  ptr(dev([0, 2])), ptr(dev([0, 1])), 1, agg, None, None, k, ptr(out), None, None, m._stream())
        assert rc != 0, (dim, k, agg)
        with pytest.raises(pa._lib.PoiError):
            m.ctx.check(rc)
    assert m.ctx.take_bad_ids() == 0
