"""-m gpu tests of the diversified recommendation (poi_diverse_pool / poi_diverse_rerank / poi_diverse_topk ->
models.compute_sub_topk_diverse, Session.recommend_diverse): the pool against the float64 oracle of tests/diverse_oracle.py with the
`check` contract of tests/test_gpu_near.py, the re-rank entry on explicit CPU-built pools, both stages end to end, trade = 1, planted
ties, the launch regimes, sessions and the explicit-score path, and the contract.  The problems are those of tests/diverse_cases.py;
tests/test_diverse_cpu.py holds them to clear gaps under the oracle alone.

The re-rank is float64 on both sides: the picks are compared exactly on every row whose oracle objectives are at least 1e-9 apart
(DC.GAP; the two sides differ by a few ulp in sin / asin / sqrt / exp and in the order of a dot product, ~1e-14), the objectives to
1e-12 absolute."""
import numpy as np
import pytest

from tests import diverse_cases as DC
from tests import diverse_oracle as DO
from tests import near_oracle as NO
from tests.test_gpu_near import AL, check

pytestmark = pytest.mark.gpu

K = DC.K
S_KM = DC.SCALE_KM
PLAN = ("diverse_path", "diverse_splits", "diverse_split_max")


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def dev(m, v, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).to(m.device)


def dev_ex(m, ex):
    return (None, None) if ex[0] is None else (dev(m, ex[0], np.int32), dev(m, ex[1], np.int32))


def same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def model_rows(m, rows):
    """(users, items, kdim, term) as compute_sub_topk_diverse hands them to the library."""
    ids, users, lo = m._users_rows(rows)
    items = m._items() if hasattr(m, "_items") else m.trained_items.t
    return users.contiguous(), items, m.kdim, m._rank_term(ids, lo)


def raw_pool(pa, m, rows, pool, ex=(None, None)):
    """poi_diverse_pool on the model's own rows -> (pool_idx, pool_score, counts) device tensors."""
    import torch
    ptr = pa.models._ptr
    users, items, kdim, term = model_rows(m, rows)
    n = users.shape[0]
    wd = sts = lp = coords = cphi = thr = None
    n_dist, dd_m = 0, 0.0
    if term is not None:
        wd, sts, lp = term
        coords, cphi, thr, n_dist, dd_m = m.coords, m._cphi, m._binthr, m.n_dist, m.dd * 1000.0
    eo, ei = dev_ex(m, ex)
    pi = torch.empty((n, pool), dtype=torch.int32, device=m.device)
    ps = torch.empty((n, pool), dtype=torch.float32, device=m.device)
    cnt = torch.empty(n, dtype=torch.int32, device=m.device)
    m.ctx.check(m.lib.poi_diverse_pool(m.ctx.handle, ptr(users), ptr(items), n, m.n_item, kdim, ptr(wd), ptr(sts), ptr(coords), ptr(cphi), ptr(thr),
                                       ptr(lp), int(n_dist), float(dd_m), ptr(eo), ptr(ei), pool, ptr(pi), ptr(ps), ptr(cnt), m._stream()))
    return pi, ps, cnt


def raw_rerank(pa, m, pi, ps, k, trade, g, items="model", scale=S_KM, check_rc=True):
    """poi_diverse_rerank on device pools -> (idx, score, pos, obj) device tensors (or the return code)."""
    import torch
    ptr = pa.models._ptr
    n, pool = pi.shape
    if items == "model":
        items = m._items() if hasattr(m, "_items") else m.trained_items.t
    idx = torch.empty((n, k), dtype=torch.int32, device=m.device)
    sc = torch.empty((n, k), dtype=torch.float32, device=m.device)
    pos = torch.empty((n, k), dtype=torch.int32, device=m.device)
    obj = torch.empty((n, k), dtype=torch.float64, device=m.device)
    rc = m.lib.poi_diverse_rerank(m.ctx.handle, ptr(pi), ptr(ps), n, pool, ptr(items) if g < 1.0 else None, m.n_item,
                                  items.shape[1] if items is not None else 0, ptr(m.coords) if g > 0.0 else None, ptr(m._cphi) if g > 0.0 else None,
                                  k, trade, g, scale, ptr(idx), ptr(sc), ptr(pos), ptr(obj), m._stream())
    if not check_rc:
        return rc
    m.ctx.check(rc)
    return idx, sc, pos, obj


def diverse(m, rows, k=K, **kw):
    """-> (idx, scores, objective, (pool ids, pool scores), counts)"""
    return m.compute_sub_topk_diverse(rows, k, scale_km=S_KM, return_scores=True, return_objective=True, return_pool=True, return_counts=True, **kw)


def build_rank_model(pa, R):
    """The case's model; on the spatial case the rows of NO_LAST lose their last POI in the scoring snapshot."""
    m = R["C"]["build"](pa)
    if R["C"]["kind"] == "spatial":
        m._last_poi[list(DC.NO_LAST)] = -1
    return m


def check_rerank(out, pi, ps, items, coords, k, trade, g, what, min_ok=0.98, every_row=False):
    """The GPU's picks against the oracle's re-ranking of the SAME pool: exact on every row with clear objective gaps."""
    idx, sc, obj = (t.cpu().numpy() for t in out[:3])
    pi, ps = np.asarray(pi, np.int64), np.asarray(ps, np.float64)
    oid, opos, oobj, gap = DO.rerank(pi, ps, items, coords, k, trade, g, S_KM)
    ok = np.ones(len(gap), bool) if every_row else gap >= DC.GAP
    print("%s: %.1f %% of %d rows have min_gap >= %g (smallest %.3g)" % (what, 100 * ok.mean(), len(ok), DC.GAP, gap.min(initial=np.inf)))
    assert ok.mean() >= min_ok, what
    assert np.array_equal(idx[ok], oid[ok]), what
    live = ok[:, None] & (oid >= 0)
    assert np.abs(obj[live] - oobj[live]).max(initial=0.0) <= 1e-12, what
    assert np.all(np.isneginf(obj[oid < 0])) and np.all(np.isneginf(sc[oid < 0])) and np.all(idx[oid < 0] == -1), what
    at = np.where(opos >= 0, opos, 0)
    assert np.array_equal(sc[live], np.float32(np.take_along_axis(ps, at, axis=1))[live]), what + ": the scores are not the pool's"
    return oid, opos, oobj, gap


# ---- 1: the pool against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", DC.RANK_CASES)
def test_pool_matches_the_oracle(pa, kind, dim):
    import torch
    R = DC.rank_case(kind, dim)
    m = build_rank_model(pa, R)
    assert m.kdim == {"bpr": dim, "spatial": 64 if dim < 64 else dim, "fpmc": 2 * dim}[kind]
    rows = np.arange(DC.N_USER)
    has_last = np.ones(DC.N_USER, bool)
    if kind == "spatial":
        has_last[list(DC.NO_LAST)] = False           # (poi_score_rank scores such a row from POI 0: not the same definition)
    for pool in DC.POOLS:
        for name, ex in (("", (None, None)), (", lists", R["ex"])):
            out = raw_pool(pa, m, rows, pool, ex)
            mask = DC.mask_of(DC.N_USER, DC.N_ITEM, ex)
            check(out, R["sc"], mask, pool, "%s dim %d pool %d%s" % (kind, dim, pool, name))
            if pool != 64:
                continue
            # the same product routine: bitwise the scores poi_score_rank gives the same ids
            pi, ps, cnt = out
            for c0 in range(0, pool, 8):
                rank, s2 = m.compute_sub_target_rank(rows, targets=pi[:, c0:c0 + 8].contiguous(), exclude=None if ex[0] is None else ex, return_scores=True)
                assert torch.equal(s2[has_last], ps[:, c0:c0 + 8][has_last]), "the scores differ from poi_score_rank's"
                assert np.array_equal(rank.cpu().numpy()[has_last], np.tile(np.arange(c0, c0 + 8), (DC.N_USER, 1))[has_last])
    assert m.ctx.take_bad_ids() == 0


def test_pool_on_a_half_table(pa):
    H = DC.half_case()
    import torch
    m = H["build"](pa)
    assert m.trained_items.t.dtype == torch.float16
    rows = np.arange(DC.N_USER)
    for pool in (33, 64):
        check(raw_pool(pa, m, rows, pool, H["ex"]), H["sc"], DC.mask_of(DC.N_USER, DC.N_ITEM, H["ex"]), pool, "half pool %d" % pool)


def tiny_model(pa, Y, n_item):
    T = Y["T"]
    m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=AL, n_user=T["n_user"], n_item=n_item, n_in=8, n_hidden=8,
                         init=dict(ux=Y["users"], lt=Y["items"]))
    m.update_trained_items(); m.update_trained_users(); m.set_coords(Y["coords"])
    return m


@pytest.mark.parametrize("n_item", [13, 5])
def test_tiny_tables(pa, n_item):
    Y = DC.tiny_case(n_item)
    m = tiny_model(pa, Y, n_item)
    rows = np.arange(6)
    mask = DC.mask_of(6, n_item, Y["ex"])
    for pool in (20, 64):
        pi, ps, cnt = check(raw_pool(pa, m, rows, pool, Y["ex"]), Y["sc"], mask, pool, "tiny %d pool %d" % (n_item, pool))
        assert cnt.tolist() == [n_item, n_item - 2, n_item, 0, n_item - 1, n_item]
        assert np.all(pi[3] == -1) and np.all(pi[0, :n_item] >= 0) and np.all(pi[0, n_item:] == -1) and np.all(np.isneginf(ps[0, n_item:]))
    for trade, g in DC.E2E:
        out = diverse(m, rows, pool=64, trade=trade, geo_weight=g, exclude=Y["ex"])
        pi, ps = (t.cpu().numpy() for t in out[3])
        oid = check_rerank(out, pi, ps, Y["items"], Y["coords"], K, trade, g, "tiny %d trade %g geo %g" % (n_item, trade, g), min_ok=1.0)[0]
        assert (oid[0] >= 0).sum() == min(K, n_item) and np.all(oid[3] == -1)


# ---- 2: the re-rank entry on explicit pools ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [20, 256])
def test_rerank_entry_on_explicit_pools(pa, dim):
    P = DC.explicit_pools(dim)
    m = DC.rank_case("bpr", dim)["C"]["build"](pa)
    pi, ps = dev(m, P["idx"], np.int32), dev(m, P["score"], np.float32)
    for k, trade, g in DC.RERANK_GRID:
        idx, sc, pos, obj = raw_rerank(pa, m, pi, ps, k, trade, g)
        oid, opos, oobj, gap = check_rerank((idx, sc, obj), P["idx"], P["score"], P["items"], P["coords"], k, trade, g,
                                            "explicit dim %d k %d trade %g geo %g" % (dim, k, trade, g), every_row=True)
        assert np.array_equal(pos.cpu().numpy(), opos)
        for r, mm in enumerate(P["m"]):
            assert (oid[r] >= 0).sum() == min(k, mm)
        assert np.all(idx.cpu().numpy()[P["m"] == 0] == -1) and np.all(pos.cpu().numpy()[P["m"] == 0] == -1)
    # narrower pools: the first 33 / 20 columns of the same rows (a full row of 33 has no -1 behind it)
    for width in (33, 20):
        sub_i, sub_s = P["idx"][:, :width].copy(), P["score"][:, :width].copy()
        idx, sc, pos, obj = raw_rerank(pa, m, dev(m, sub_i, np.int32), dev(m, sub_s, np.float32), 20, 0.7, 0.5)
        oid, opos, oobj, gap = DO.rerank(sub_i, sub_s, P["items"], P["coords"], 20, 0.7, 0.5, S_KM)
        ok = gap >= DC.GAP
        assert ok.mean() >= 0.9 and np.array_equal(idx.cpu().numpy()[ok], oid[ok]) and np.array_equal(pos.cpu().numpy()[ok], opos[ok])
    # equal scores: every rel is 1, the similarity alone decides
    flat_i, flat_s = P["idx"][-3:].copy(), np.full((3, 64), 1.5)
    idx, sc, pos, obj = raw_rerank(pa, m, dev(m, flat_i, np.int32), dev(m, flat_s, np.float32), 20, 0.3, 1.0)
    oid, opos, oobj, gap = DO.rerank(flat_i, flat_s, P["items"], P["coords"], 20, 0.3, 1.0, S_KM)
    assert gap.min() >= DC.GAP and np.array_equal(idx.cpu().numpy(), oid) and obj.cpu().numpy()[0, 0] == 0.3
    assert m.ctx.take_bad_ids() == 0


# ---- 3: end to end ---------------------------------------------------------------------------------------------------------------------
def end_to_end(pa, m, rows, sc, ex, items, coords, name, pools=((64, DC.E2E),), min_ok=0.98, every_row=False):
    for pool, params in pools:
        for trade, g in params:
            what = "%s pool %d trade %g geo %g" % (name, pool, trade, g)
            out = diverse(m, rows, pool=pool, trade=trade, geo_weight=g, exclude=None if ex[0] is None else ex)
            pi, ps = out[3]
            check((pi, ps, out[4]), sc, DC.mask_of(len(sc), sc.shape[1], ex), pool, what)
            check_rerank(out, pi.cpu().numpy(), ps.cpu().numpy(), items, coords, K, trade, g, what, min_ok=min_ok, every_row=every_row)
            # the two entries, composed by hand, give the same bits
            p2 = raw_pool(pa, m, rows, pool, ex)
            assert same(p2, (pi, ps, out[4])), what + ": poi_diverse_pool differs"
            r2 = raw_rerank(pa, m, p2[0], p2[1], K, trade, g)
            assert same((r2[0], r2[1], r2[3]), out[:3]), what + ": poi_diverse_pool + poi_diverse_rerank differs from poi_diverse_topk"


@pytest.mark.parametrize("kind,dim", DC.RANK_CASES)
def test_end_to_end(pa, kind, dim):
    R = DC.rank_case(kind, dim)
    m = build_rank_model(pa, R)
    rows = np.arange(DC.N_USER)
    pools = ((64, DC.E2E),) + (((20, DC.E2E[:1]), (33, DC.E2E[:1])) if (kind, dim) == ("bpr", 128) else ())
    end_to_end(pa, m, rows, R["sc"], R["ex"], R["items"], R["coords"], "%s dim %d, lists" % (kind, dim), pools)
    end_to_end(pa, m, rows, R["sc"], (None, None), R["items"], R["coords"], "%s dim %d" % (kind, dim), ((64, DC.E2E[:1]),))
    assert m.ctx.take_bad_ids() == 0


def test_end_to_end_on_a_half_table(pa):
    H = DC.half_case()
    m = H["build"](pa)
    end_to_end(pa, m, np.arange(DC.N_USER), H["sc"], H["ex"], H["items"], H["coords"], "half")


# ---- 4: trade = 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128)])
def test_trade_one_is_the_plain_top_k(pa, kind, dim):
    import torch
    R = DC.rank_case(kind, dim)
    m = R["C"]["build"](pa)                                  # (every row keeps its last POI: compute_sub_topk is the reference)
    rows = np.arange(DC.N_USER)
    sc = DC.case_scores(R["C"], DC.last_of(R["C"]["T"]))
    for g in (1.0, 0.5):
        idx, s, obj, (pi, ps), cnt = diverse(m, rows, pool=64, trade=1.0, geo_weight=g)
        assert torch.equal(idx, pi[:, :K]) and torch.equal(s, ps[:, :K])
        assert obj[:, 0].eq(1.0).all() and (obj[:, 1:] <= obj[:, :-1]).all()
    ok = NO.qualifying(sc, np.ones_like(sc, bool), 64)
    assert ok.mean() >= 0.9
    top = m.compute_sub_topk(rows, K).cpu().numpy()
    assert np.array_equal(idx.cpu().numpy()[ok], top[ok])


# ---- 5: planted ties -----------------------------------------------------------------------------------------------------------------------
def test_planted_ties(pa):
    Tc = DC.tie_case()
    m = Tc["C"]["build"](pa)
    rows = np.arange(DC.N_USER)
    trade = 0.9
    a = m.compute_sub_topk_diverse(rows, 32, pool=64, trade=trade, geo_weight=1.0, scale_km=S_KM, return_scores=True, return_objective=True, return_pool=True)
    b = m.compute_sub_topk_diverse(rows, 32, pool=64, trade=trade, geo_weight=1.0, scale_km=S_KM, return_scores=True, return_objective=True, return_pool=True)
    assert same(a[:3] + a[3], b[:3] + b[3]), "two identical calls differ"
    idx, sc, obj = (t.cpu().numpy() for t in a[:3])
    pi, ps = (t.cpu().numpy() for t in a[3])
    seen = both = 0
    for lo, hi in DC.TWINS:
        for r in rows:
            at = np.nonzero(pi[r] == lo)[0]
            if len(at) == 0 or at[0] == 63:
                continue
            seen += 1
            assert pi[r, at[0] + 1] == hi and ps[r, at[0]] == ps[r, at[0] + 1], "the twins enter the pool in id order"
            t_lo, t_hi = np.nonzero(idx[r] == lo)[0], np.nonzero(idx[r] == hi)[0]
            if len(t_lo) and len(t_hi):
                both += 1
                assert t_lo[0] < t_hi[0], "equal objectives go to the lower position"
                rel = (np.float64(ps[r, at[0]]) - ps[r, 63]) / (np.float64(ps[r, 0]) - ps[r, 63])
                assert abs(obj[r, t_hi[0]] - (trade * rel - (1.0 - trade) * 1.0)) <= 1e-12, "the second twin carries pen = 1"
    assert seen >= 20 and both >= 5, (seen, both)
    # exact ties are decided by the position on both sides: every row against the oracle
    check_rerank(a, pi, ps, Tc["items"], Tc["coords"], 32, trade, 1.0, "ties", every_row=True)


# ---- 6: launch regimes -----------------------------------------------------------------------------------------------------------------------
def test_both_regimes_and_every_split_give_the_same_bits(pa):
    W = DC.wide_case()
    m = W["C"]["build"](pa)
    rows = np.arange(300)
    default = 256
    flat = lambda o: o[:3] + o[3] + (o[4],)
    run = lambda r, ex: flat(diverse(m, r, pool=64, trade=0.7, geo_weight=0.5, exclude=ex))
    sub_ex = lambda r: (W["ex"][0][r:r + 2] - W["ex"][0][r], W["ex"][1][W["ex"][0][r]:W["ex"][0][r + 1]])
    try:
        ref = run(rows, W["ex"])                              # 300 rows: above the switch point
        assert {k: m.ctx.last_plan(k) for k in PLAN} == dict(diverse_path=0, diverse_splits=0, diverse_split_max=default)
        check((ref[3], ref[4], ref[5]), W["sc"], DC.mask_of(300, DC.N_ITEM, W["ex"]), 64, "wide")
        check_rerank(ref, ref[3].cpu().numpy(), ref[4].cpu().numpy(), W["items"], W["coords"], K, 0.7, 0.5, "wide")
        assert same(run(rows, W["ex"]), ref), "two identical calls differ"
        for grid in (1, 2, 7, 64):
            m.ctx.set_option("diverse_split_max", 1 << 30); m.ctx.set_option("diverse_grid", grid)
            out = run(rows, W["ex"])
            assert {k: m.ctx.last_plan(k) for k in PLAN} == dict(diverse_path=1, diverse_splits=grid, diverse_split_max=1 << 30)
            assert same(out, ref), "grid %d differs from the tile path" % grid
        m.ctx.set_option("diverse_split_max", default); m.ctx.set_option("diverse_grid", 0)
        for r in (0, 31, 32, 150, 299):                      # a row alone (the split path chooses its own slices) against the call of 300
            alone = run(np.array([r]), sub_ex(r))
            plan = {k: m.ctx.last_plan(k) for k in PLAN}
            assert plan["diverse_path"] == 1 and 2 <= plan["diverse_splits"] <= 64, plan
            assert same(alone, tuple(t[r:r + 1] for t in ref)), "row %d alone differs" % r
        m.ctx.set_option("diverse_split_max", 0)             # ... and the first 40 rows as a call of their own, forced onto the tile path
        sub = run(rows[:40], (W["ex"][0][:41], W["ex"][1][:W["ex"][0][40]]))
        assert m.ctx.last_plan("diverse_path") == 0 and same(sub, tuple(t[:40] for t in ref))
    finally:
        m.ctx.set_option("diverse_split_max", default); m.ctx.set_option("diverse_grid", 0)


# ---- 7: sessions and the explicit-score path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "lstm"])
def test_session_recommend_diverse_is_the_model_path_on_the_same_states(pa, kind):
    import torch
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    if kind == "spatial":
        m = TS.spatial_model(pa, T, TS.spatial_init(32, T))
        s = m.session(n_slot=T["n_user"])
    else:
        m = TC.model(pa, "lstm", T, TC.params("lstm", 60, T))
        m.set_coords(T["coords"])
        s = m.cell_session(n_slot=T["n_user"])
    slots = np.arange(T["n_user"])
    for t in range(3):
        s.advance(slots, T["train"][0][:, t])
    ex = DC.exclusion_lists(14, T["n_user"], T["n_item"])
    kw = dict(pool=64, trade=0.7, geo_weight=0.5, scale_km=S_KM, return_scores=True, return_objective=True, return_pool=True, return_counts=True)
    got = s.recommend_diverse(slots, K, exclude=ex, **kw)
    st = s.state()
    # the same states through the model: its user rows, bin probabilities and last POIs replaced by the session's
    m.update_trained_users(torch.as_tensor(np.float32(st["h"])))
    if kind == "spatial":
        m.update_trained_sus(torch.as_tensor(st["sts"]))
        m._last_poi = dev(m, st["last_poi"], np.int32)
    want = m.compute_sub_topk_diverse(slots, K, exclude=ex, **kw)
    flat = lambda o: o[:3] + o[3] + (o[4],)
    assert same(flat(got), flat(want))
    last = s.recommend_diverse(slots[:5], K, exclude="last", return_counts=True)
    assert np.all(last[1].cpu().numpy() == T["n_item"] - 1) and not np.any(last[0].cpu().numpy() == st["last_poi"][:5, None])
    with pytest.raises(ValueError):
        s.recommend_diverse(slots, K, exclude="train")
    with pytest.raises(ValueError):
        s.recommend_diverse(slots, K, pool=10)


def test_explicit_score_path_through_prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(45, 700, 14, 4)
    m = _model(ds)
    m.update_trained_items()
    m.set_coords(np.asarray(ds.coords, np.float64)[:ds.n_item])
    users = np.arange(ds.n_user)
    full = np.float64(m.compute_sub_all_scores(users).reshape(ds.n_user, -1, ds.n_item)[:, 0])       # row 0: the query is the last train POI
    ex = DC.exclusion_lists(5, ds.n_user, ds.n_item)
    mask = DC.mask_of(ds.n_user, ds.n_item, ex)
    out = diverse(m, users, pool=64, trade=0.7, geo_weight=1.0, exclude=ex)
    pi, ps = out[3]
    check((pi, ps, out[4]), full, mask, 64, "prme pool")
    check_rerank(out, pi.cpu().numpy(), ps.cpu().numpy(), None, np.asarray(ds.coords, np.float64), K, 0.7, 1.0, "prme")
    with pytest.raises(ValueError, match="geo_weight=1"):
        m.compute_sub_topk_diverse(users, K, geo_weight=0.5)


def test_carnn_session_takes_the_explicit_score_path(pa):
    from tests.test_gpu_group import carnn_model
    m = carnn_model(pa)
    s = m.cell_session(n_slot=21)
    rng = np.random.default_rng(4)
    slots = np.arange(20)                                    # slot 20 never checks in
    for t in range(3):
        s.advance(slots, rng.integers(0, 150, 20))
    every = np.arange(21)
    pool_i, pool_s = s.recommend(every, 64, return_scores=True)
    idx, sc, obj, (pi, ps), cnt = s.recommend_diverse(every, K, pool=64, trade=0.7, geo_weight=0.5, scale_km=S_KM, return_scores=True,
                                                      return_objective=True, return_pool=True, return_counts=True)
    assert np.all(idx[20].cpu().numpy() == -1) and cnt[20] == 0 and np.all(cnt[:20].cpu().numpy() == 150)
    assert np.array_equal(pi[:20].cpu().numpy(), pool_i[:20].cpu().numpy()) and np.array_equal(ps[:20].cpu().numpy(), pool_s[:20].cpu().numpy())
    items = np.float64(m.trained_items.get_value())
    check_rerank((idx[:20], sc[:20], obj[:20]), pi[:20].cpu().numpy(), ps[:20].cpu().numpy(), items, m.coords.cpu().numpy(), K, 0.7, 0.5, "carnn session",
                 min_ok=0.9)


# ---- 8: the contract -----------------------------------------------------------------------------------------------------------------------
def test_contract(pa):
    import torch
    R = DC.rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    rows = np.arange(DC.N_USER)
    ptr = pa.models._ptr
    flat = lambda o: tuple(t.cpu().numpy() for t in o[:3] + o[3] + (o[4],))
    clean = flat(diverse(m, rows, pool=64, exclude=R["ex"]))
    # a malformed exclusion list (device lists: the kernel's to find): ids not ascending / out of range
    eo, ei = R["ex"]
    r_x = int(np.nonzero(np.diff(eo) >= 2)[0][0])
    for make in (lambda e: e.__setitem__(slice(eo[r_x], eo[r_x] + 2), e[eo[r_x]:eo[r_x] + 2][::-1].copy()), lambda e: e.__setitem__(eo[r_x + 1] - 1, DC.N_ITEM)):
        e2 = ei.copy(); make(e2)
        bad_ex = (dev(m, eo, np.int32), dev(m, e2, np.int32))
        with pytest.raises(IndexError):
            m.compute_sub_topk_diverse(rows, K, exclude=bad_ex)
        got = flat(diverse(m, rows, pool=64, exclude=bad_ex, sync=False))
        assert m.ctx.take_bad_ids() == 1
        assert np.all(got[0][r_x] == -1) and np.all(np.isneginf(got[1][r_x])) and np.all(got[3][r_x] == -1) and got[5][r_x] == 0
        good = rows != r_x
        assert all(np.array_equal(x[good], y[good]) for x, y in zip(got, clean)), "the other rows changed"
    for bad_host in ((eo, np.where(np.arange(len(ei)) == eo[r_x], DC.N_ITEM, ei)), (eo[::-1].copy(), ei)):
        with pytest.raises((IndexError, ValueError)):
            m.compute_sub_topk_diverse(rows, K, exclude=bad_host)
    assert m.ctx.take_bad_ids() == 0
    # NaN and +-inf scores are never pooled: planted values on the explicit-score path (poi_topk + poi_diverse_rerank)
    sc = np.float32(R["sc"][:8]).copy()
    sc[0, :5] = np.nan; sc[1, 7] = np.inf; sc[1, 9] = -np.inf; sc[2, :] = np.nan; sc[3, 10:] = -np.inf
    full = dev(m, sc, np.float32)
    sim = m._diverse_sim(0.5, m.trained_items.t)
    idx, obj, (pi, ps), cnt = m._diverse_from_scores(lambda o, c: full[o:o + c], 8, (None, None), sim, K, 64, 0.7, 0.5, S_KM, False, True, True, True, True)
    pi_h, ps_h = pi.cpu().numpy(), ps.cpu().numpy()
    opi, ops, ocnt = DO.pool(np.float64(sc), np.ones(sc.shape, bool), 64)
    assert np.array_equal(pi_h, opi) and np.array_equal(ps_h, np.float32(ops)) and np.all(cnt.cpu().numpy() == DC.N_ITEM)
    assert np.all(pi_h[2] == -1) and np.all(idx[2].cpu().numpy() == -1) and (pi_h[3] >= 0).sum() == 10 and (idx[3].cpu().numpy() >= 0).sum() == 10
    assert not set(pi_h[0].tolist()) & set(range(5)) and 7 not in pi_h[1] and 9 not in pi_h[1]
    # a pool id outside the table: the row is rejected, counted once
    P = DC.explicit_pools(20)
    bad_pool = P["idx"].copy(); bad_pool[-1, 3] = DC.N_ITEM
    out = raw_rerank(pa, m, dev(m, bad_pool, np.int32), dev(m, P["score"], np.float32), K, 0.7, 0.5)
    assert m.ctx.take_bad_ids() == 1 and np.all(out[0][-1].cpu().numpy() == -1) and np.all(out[2][-1].cpu().numpy() == -1)
    # n = 0 is a no-op; sizes and error codes
    assert m.compute_sub_topk_diverse(np.zeros(0, np.int64), K).shape == (0, K)
    pi, ps = dev(m, P["idx"], np.int32), dev(m, P["score"], np.float32)
    out32 = torch.empty((21, K), dtype=torch.int32, device=m.device)
    lib, h, st = m.lib, m.ctx.handle, m._stream()
    for k, trade, g, scale in ((0, 0.7, 1.0, 1.0), (33, 0.7, 1.0, 1.0), (K, -0.1, 1.0, 1.0), (K, 1.5, 1.0, 1.0), (K, 0.7, 1.5, 1.0), (K, 0.7, -0.5, 1.0),
                               (K, 0.7, 1.0, 0.0), (K, float("nan"), 1.0, 1.0)):
        rc = lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 21, 64, ptr(m.trained_items.t), DC.N_ITEM, 20, ptr(m.coords), ptr(m._cphi), k, trade, g, scale,
                                    ptr(out32), None, None, None, st)
        assert rc == (-4 if k in (0, 33) else -1), (k, trade, g, scale, rc)      # POI_ENOTSUP / POI_EINVAL
        with pytest.raises(pa._lib.PoiError):
            m.ctx.check(rc)
    # coords missing with geo_weight > 0, items missing with geo_weight < 1, pool < k, dim not a multiple of 4
    assert lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 21, 64, None, DC.N_ITEM, 0, None, None, K, 0.7, 1.0, 1.0, ptr(out32), None, None, None, st) != 0
    assert lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 21, 64, None, DC.N_ITEM, 20, ptr(m.coords), ptr(m._cphi), K, 0.7, 0.5, 1.0, ptr(out32), None, None, None, st) != 0
    assert lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 21, 16, None, DC.N_ITEM, 0, ptr(m.coords), ptr(m._cphi), K, 0.7, 1.0, 1.0, ptr(out32), None, None, None, st) != 0
    assert lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 21, 64, ptr(m.trained_items.t), DC.N_ITEM, 18, None, None, K, 0.7, 0.0, 1.0, ptr(out32), None, None, None, st) != 0
    users = m.trained_users.t
    for dim, pool in ((18, 64), (20, 65), (20, 0)):
        assert lib.poi_diverse_pool(h, ptr(users), ptr(m.trained_items.t), 4, DC.N_ITEM, dim, None, None, None, None, None, None, 0, 0.0, None, None, pool,
                                    ptr(pi), ptr(ps), None, st) != 0, (dim, pool)
    assert lib.poi_diverse_pool(h, ptr(users), ptr(m.trained_items.t), 0, DC.N_ITEM, 20, None, None, None, None, None, None, 0, 0.0, None, None, 64,
                                ptr(pi), ptr(ps), None, st) == 0
    assert lib.poi_diverse_rerank(h, ptr(pi), ptr(ps), 0, 64, None, DC.N_ITEM, 0, ptr(m.coords), ptr(m._cphi), K, 0.7, 1.0, 1.0, ptr(out32), None, None, None, st) == 0
    for bad in (dict(k=33), dict(pool=65), dict(trade=2.0), dict(geo_weight=-1.0), dict(scale_km=0.0)):
        with pytest.raises(ValueError):
            m.compute_sub_topk_diverse(rows, **dict(dict(k=K), **bad))
    assert m.ctx.take_bad_ids() == 0
