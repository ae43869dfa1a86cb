"""-m gpu tests of the similar-rows entries (poi_row_inv_norms / poi_similar_topk / poi_similar_rows / poi_similar_nearest ->
models.similar_pois / similar_users / nearest_visited): places like this one, users like this one, "because you visited X".  The
ranking contract against the float64 oracle of tests/similar_oracle.py on the cases of tests/similar_cases.py (through
tests.test_gpu_near.check), the bits of the fused entry against poi_similar_rows and against poi_score_rows x the norms, symmetry,
every grid, both regimes and the rows + select route, invariance, tiny tables, exclusion edges, the contract, a zero row, twins, the
large-k route, half tables, the user side and the nearest visited POI."""
import ctypes

import numpy as np
import pytest

from tests import similar_cases as SC
from tests import similar_oracle as SO
from tests.similar_cases import GEO, K, N_ITEM, N_QUERY, N_USER
from tests.test_gpu_near import built, check

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("similar_path", "similar_splits", "similar_split_max")
SPLIT_MAX, ROWS_MAX = 16384, 1024                       # the options' defaults


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


_MODELS = {}


def model_of(pa, R, key):
    if key not in _MODELS:
        _MODELS[key] = built(pa, R["C"])[0]
    return _MODELS[key]


def sim(m, pois, k=K, **kw):
    return m.similar_pois(pois, k, return_scores=True, return_counts=True, **kw)


def fused(m, pois, k=K, **kw):
    """sim() with the rows + select route switched off: the fused walk."""
    m.ctx.set_option("similar_rows_max", 0)
    try:
        return sim(m, pois, k, **kw)
    finally:
        m.ctx.set_option("similar_rows_max", ROWS_MAX)


def same(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32)) for x, y in zip(a, b))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def geo_ptrs(m, g):
    return (vp(m.coords), vp(m._cphi)) if g > 0.0 else (None, None)


def inv_norms(m, x, n):
    import torch
    inv = torch.full((n,), float("nan"), dtype=torch.float64, device=m.device)
    m.ctx.check(m.lib.poi_row_inv_norms(m.ctx.handle, vp(x), n, x.shape[1], vp(inv), m._stream()))
    return inv


def similar_rows(m, x, n, qs, g=0.0, s=1.0, ld=None, inv=None):
    """poi_similar_rows of the queries: (n_q, ld) float32, NaN where the kernel wrote nothing."""
    import torch
    ld = ld or n
    q = torch.as_tensor(np.asarray(qs, np.int32)).to(m.device)
    out = torch.full((len(qs), ld), float("nan"), dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_similar_rows(m.ctx.handle, vp(x), n, x.shape[1], *geo_ptrs(m, g), g, s, vp(inv), vp(q), len(qs), vp(out), ld, m._stream()))
    return out.cpu().numpy()


def score_rows_self(m, x, n):
    """poi_score_rows of the table against itself: (n, n) float32, [i][j] = row x[i] against item x[j]."""
    import torch
    out = torch.empty((n, n), dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_score_rows(m.ctx.handle, vp(x), vp(x), n, n, x.shape[1], None, None, None, None, None, None, 0, 0.0, vp(out), n, m._stream()))
    return out.cpu().numpy()


# ---- 1: ranking and bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", SC.RANK_CASES)
def test_ranking_matches_the_oracle_and_the_bits_of_the_rows(pa, kind, dim):
    R = SC.poi_case(kind, dim)
    m = model_of(pa, R, (kind, dim))
    pois, x = R["pois"], m._diverse_items()
    inv = inv_norms(m, x, N_ITEM)
    full = score_rows_self(m, x, N_ITEM)
    for g, s in GEO:
        osc = SC.sim_of(kind, dim, g, s)[pois]
        rows = similar_rows(m, x, N_ITEM, pois, g, s, ld=N_ITEM + 3, inv=inv)
        assert np.isnan(rows[:, N_ITEM:]).all() and np.isneginf(rows[np.arange(N_QUERY), pois]).all()
        for name, ex, mask in (("", None, SO.candidate_mask(pois, N_ITEM)), (", lists", R["ex"], SO.candidate_mask(pois, N_ITEM, *R["ex"]))):
            out = fused(m, pois, geo_weight=g, scale_km=s, exclude=ex)       # the fused walk ...
            idx, sc, cnt = check(out, osc, mask, K, "%s dim %d g %g scale %g%s" % (kind, dim, g, s, name))
            got = np.take_along_axis(rows, np.maximum(idx, 0), axis=1)
            assert np.array_equal(bits(sc)[idx >= 0], bits(got)[idx >= 0]), "score_out differs from poi_similar_rows in some bit"
            assert same(sim(m, pois, geo_weight=g, scale_km=s, exclude=ex), out), "the default route (score rows + selection) differs"
        if g == 0.0:                                          # float32(float64(poi_score_rows bits) * (inv[i] * inv[j])), on the host
            iv = inv.cpu().numpy()
            want = (np.float64(full[pois]) * (iv[pois][:, None] * iv[None, :])).astype(np.float32) + np.float32(0.0)
            live = np.ones_like(want, bool); live[np.arange(N_QUERY), pois] = False
            assert np.array_equal(bits(rows[:, :N_ITEM])[live], bits(want)[live]), "g = 0: not the float32 product times the norms"
    assert m.ctx.take_bad_ids() == 0


def test_inverse_norms_match_the_oracle_and_a_zero_row_gives_zero(pa):
    for R, key in ((SC.zero_case(17), ("zero", 17)), (SC.poi_case("bpr", 256), ("bpr", 256)), (SC.half_case("spatial", 128), ("half", "spatial", 128))):
        m = model_of(pa, R, key)
        inv = inv_norms(m, m._diverse_items(), N_ITEM).cpu().numpy()
        want = SO.inv_norms(R["items"])
        assert np.all(np.abs(inv - want) <= 1e-14 * want), key
        assert key[0] != "zero" or (inv[17] == 0.0 and want[17] == 0.0)


@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128)])
def test_the_similarity_is_symmetric_to_the_bit(pa, kind, dim):
    R = SC.poi_case(kind, dim)
    m = model_of(pa, R, (kind, dim))
    qs = np.arange(64)                                        # a square block of queries: two query blocks against two tiles
    for g, s in GEO:
        rows = similar_rows(m, m._diverse_items(), N_ITEM, qs, g, s)[:, :64]
        assert np.array_equal(bits(rows), bits(rows.T)), "sim(i, j) and sim(j, i) differ (g %g)" % g


# ---- 2: regimes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,s", [(0.0, 1.0), (0.5, 5.0)])
def test_every_grid_both_regimes_and_the_rows_route_give_the_same_bits(pa, g, s):
    n_item = 3001                                             # 94 tiles: 64 slices are not empty
    R = SC.poi_case("bpr", 20, n_item)
    m = model_of(pa, R, ("bpr", 20, n_item))
    pois, x = R["pois"], m._diverse_items()
    plan = lambda: {k: m.ctx.last_plan(k) for k in PLAN_KEYS}
    kw = dict(geo_weight=g, scale_km=s, exclude=R["ex"])
    try:
        m.ctx.set_option("similar_rows_max", 0)               # the fused walk: 70 queries take the split regime, slices by the CUs
        ref = sim(m, pois, **kw)
        p = plan()
        assert p["similar_path"] == 1 and 1 <= p["similar_splits"] <= 64 and p["similar_split_max"] == SPLIT_MAX, p
        osc = SO.sim_matrix(R["items"], R["coords"], g, s)[pois]
        check(ref, osc, SO.candidate_mask(pois, n_item, *R["ex"]), K, "default plan g %g" % g)
        rows = similar_rows(m, x, n_item, pois, g, s)
        for grid in (1, 2, 3, 7, 64):
            m.ctx.set_option("similar_split_max", 1 << 30); m.ctx.set_option("similar_grid", grid)
            out = sim(m, pois, **kw)
            assert plan() == dict(similar_path=1, similar_splits=grid, similar_split_max=1 << 30)
            assert same(out, ref), "grid %d differs" % grid
            assert np.array_equal(bits(similar_rows(m, x, n_item, pois, g, s)), bits(rows)), "rows: grid %d differs" % grid
        m.ctx.set_option("similar_split_max", 0); m.ctx.set_option("similar_grid", 0)
        out = sim(m, pois, **kw)
        assert plan() == dict(similar_path=0, similar_splits=0, similar_split_max=0)
        assert same(out, ref), "one workgroup per query block differs from the slices"
        assert np.array_equal(bits(similar_rows(m, x, n_item, pois, g, s)), bits(rows))
        m.ctx.set_option("similar_split_max", SPLIT_MAX); m.ctx.set_option("similar_rows_max", ROWS_MAX)
        out = sim(m, pois, **kw)                              # the default: k = 20 through the score rows and the selection
        assert plan()["similar_path"] == 2
        assert same(out, ref), "the rows + select route differs from the fused walk"
        m.ctx.set_option("similar_rows_max", 69)              # one query fewer than the call has: the fused walk again
        assert same(sim(m, pois, **kw), ref) and plan()["similar_path"] == 1
        one = sim(m, pois[:1], **dict(kw, exclude=None))      # one query
        assert plan()["similar_path"] == 2
        m.ctx.set_option("similar_rows_max", 0)
        assert same(sim(m, pois[:1], **dict(kw, exclude=None)), one) and plan()["similar_path"] == 1
    finally:
        m.ctx.set_option("similar_split_max", SPLIT_MAX); m.ctx.set_option("similar_grid", 0); m.ctx.set_option("similar_rows_max", ROWS_MAX)
    assert m.ctx.take_bad_ids() == 0


# ---- 3: invariance ---------------------------------------------------------------------------------------------------------------------
def test_a_query_does_not_depend_on_its_call(pa):
    R = SC.poi_case("spatial", 128)
    m = model_of(pa, R, ("spatial", 128))
    pois = R["pois"]
    off, ids = R["ex"]
    kw = dict(geo_weight=0.5, scale_km=5.0)
    ref = sim(m, pois, exclude=R["ex"], **kw)
    part = lambda a, b: (off[a:b + 1] - off[a], ids[off[a]:off[b]])
    for q in (0, 1, 31, 32, 63, 64, 69):                      # alone (the rows + select route) against the same query inside the call of 70
        assert same(sim(m, pois[q:q + 1], exclude=part(q, q + 1), **kw), tuple(t[q:q + 1] for t in ref)), "query %d alone differs" % q
    try:
        for rows_max in (ROWS_MAX, 0):
            m.ctx.set_option("similar_rows_max", rows_max)
            for n_q in (1, 31, 32, 33):
                assert same(sim(m, pois[:n_q], exclude=part(0, n_q), **kw), tuple(t[:n_q] for t in ref)), "the first %d queries differ" % n_q
            twice = np.array([pois[6], pois[40], pois[6]])
            out = sim(m, twice, **kw)
            assert same(tuple(t[0:1] for t in out), tuple(t[2:3] for t in out))
            assert same(tuple(t[0:1] for t in out), sim(m, pois[6:7], **kw))
    finally:
        m.ctx.set_option("similar_rows_max", ROWS_MAX)


# ---- 4: edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_item", [6, 13])
def test_tiny_tables_fill_and_count(pa, n_item):
    R = SC.poi_case("bpr", 20, n_item)
    m = model_of(pa, R, ("bpr", 20, n_item))
    pois = R["pois"]
    for g, s in ((0.0, 1.0), (0.5, 5.0)):
        osc = SO.sim_matrix(R["items"], R["coords"], g, s)[pois]
        idx, sc, cnt = check(sim(m, pois, geo_weight=g, scale_km=s), osc, SO.candidate_mask(pois, n_item), K, "%d POIs" % n_item, min_ok=0.0)
        assert np.all(cnt == n_item - 1) and np.all(idx[:, n_item - 1:] == -1) and np.all(idx[:, :n_item - 1] >= 0)
    everything = (np.arange(4) * n_item, np.tile(np.arange(n_item), 3))      # three queries whose lists exclude everything, themselves included
    idx, sc, cnt = (t.cpu().numpy() for t in sim(m, pois[:3], exclude=everything))
    assert np.all(cnt == 0) and np.all(idx == -1) and np.all(np.isneginf(sc))
    assert m.ctx.take_bad_ids() == 0


def test_a_list_that_names_the_query_does_not_subtract_it_twice(pa):
    R = SC.poi_case("bpr", 20)
    m = model_of(pa, R, ("bpr", 20))
    pois = R["pois"][:8]
    others = [int(j) for j in range(40) if j not in pois[:2]][:5]
    ex = SO.csr([sorted(others + [int(pois[0])]), others, [int(pois[2])], [], [], [], [], []])
    try:
        for rows_max in (ROWS_MAX, 0):                        # the rows + select route (8 queries) and the fused walk
            m.ctx.set_option("similar_rows_max", rows_max)
            for k in (K, 40):
                idx, sc, cnt = (t.cpu().numpy() for t in sim(m, pois, k, exclude=ex))
                assert cnt.tolist() == [N_ITEM - 6, N_ITEM - 6, N_ITEM - 1] + [N_ITEM - 1] * 5, (rows_max, k, cnt)
                assert not np.isin(idx[0], others + [pois[0]]).any() and not (idx == pois[:, None]).any()
    finally:
        m.ctx.set_option("similar_rows_max", ROWS_MAX)


def test_contract(pa):
    import torch
    R = SC.poi_case("bpr", 20)
    m = model_of(pa, R, ("bpr", 20))
    pois = R["pois"]
    off, ids = R["ex"]
    dev = lambda v: torch.as_tensor(np.asarray(v, np.int32)).to(m.device)
    for bad in ([N_ITEM], [-1], [3, N_ITEM + 5]):             # host ids out of range raise before the launch
        with pytest.raises(IndexError):
            m.similar_pois(bad, K)
    with pytest.raises(IndexError):
        m.similar_pois(pois[:2], K, exclude=([0, 1, 2], [0, N_ITEM]))
    with pytest.raises(ValueError):
        m.similar_pois(pois[:2], K, exclude=([0, 2, 4], [5, 3, 1, 2]))
    with pytest.raises(ValueError):
        m.similar_pois(pois, K, exclude="train")
    for k in (0, N_ITEM, 5000):
        with pytest.raises(ValueError):
            m.similar_pois(pois, k)
    for g in (1.0, -0.5):
        with pytest.raises(ValueError):
            m.similar_pois(pois, K, geo_weight=g)
    assert m.ctx.take_bad_ids() == 0
    # device tensors: a bad query id and a broken list are the kernel's to find - rejected, counted once, IndexError with sync
    q = pois[:8].copy(); q[5] = N_ITEM
    e8 = (off[:9], ids[:off[8]])
    assert off[3] - off[2] >= 2
    try:
        for rows_max in (ROWS_MAX, 0):
            m.ctx.set_option("similar_rows_max", rows_max)
            clean = tuple(t.cpu().numpy() for t in sim(m, pois[:8], exclude=e8))
            with pytest.raises(IndexError):
                m.similar_pois(dev(q), K, exclude=e8)
            for k in (K, 40):                                 # the C entry, and the similarity rows + selection of the large-k route
                ref = tuple(t.cpu().numpy() for t in sim(m, pois[:8], k, exclude=e8))
                idx, sc, cnt = (t.cpu().numpy() for t in sim(m, dev(q), k, exclude=e8, sync=False))
                assert m.ctx.take_bad_ids() == 1
                assert np.all(idx[5] == -1) and np.all(np.isneginf(sc[5])) and cnt[5] == 0
                good = np.arange(8) != 5
                assert all(np.array_equal(x[good], y[good]) for x, y in zip((idx, sc, cnt), ref)), "the other queries changed"
            for breaker in (lambda e: e.__setitem__(off[2] + 1, e[off[2]]), lambda e: e.__setitem__(off[3] - 1, N_ITEM)):
                e = ids[:off[8]].copy(); breaker(e)
                idx, sc, cnt = (t.cpu().numpy() for t in sim(m, dev(pois[:8]), exclude=(dev(off[:9]), dev(e)), sync=False))
                assert m.ctx.take_bad_ids() == 1
                assert np.all(idx[2] == -1) and np.all(np.isneginf(sc[2])) and cnt[2] == 0
                good = np.arange(8) != 2
                assert all(np.array_equal(x[good], y[good]) for x, y in zip((idx, sc, cnt), clean))
                with pytest.raises(IndexError):
                    sim(m, dev(pois[:8]), exclude=(dev(off[:9]), dev(e)))
    finally:
        m.ctx.set_option("similar_rows_max", ROWS_MAX)
    rows = similar_rows(m, m._diverse_items(), N_ITEM, q)     # poi_similar_rows: the row of a rejected query is -inf, counted once
    assert m.ctx.take_bad_ids() == 1 and np.all(np.isneginf(rows[5])) and np.isfinite(np.delete(rows, 5, axis=0)).sum() == 7 * (N_ITEM - 1)
    # the C entry: k = 33 is not supported, g = 1 is refused
    x = m._diverse_items()
    out = torch.empty((8, 33), dtype=torch.int32, device=m.device)
    q8 = dev(pois[:8])
    call = lambda g, k: m.lib.poi_similar_topk(m.ctx.handle, vp(x), N_ITEM, x.shape[1], vp(m.coords), vp(m._cphi), g, 1.0, None, vp(q8), 8,
                                               None, None, k, vp(out), None, None, m._stream())
    assert call(0.5, 33) == -4                                # POI_ENOTSUP
    with pytest.raises(pa._lib.PoiError, match="k <= 32"):
        m.ctx.check(call(0.5, 33))
    with pytest.raises(pa._lib.PoiError, match="geo_weight"):
        m.ctx.check(call(1.0, 20))
    assert m.ctx.take_bad_ids() == 0


def test_a_zero_row_has_no_embedding_similarity_and_is_still_ranked_by_geo(pa):
    z = 17
    R = SC.zero_case(z)
    m = model_of(pa, R, ("zero", z))
    x = m._diverse_items()
    rows = similar_rows(m, x, N_ITEM, [z, 5])
    assert np.all(np.delete(rows[0], z) == 0.0) and rows[1, z] == 0.0 and np.isneginf(rows[0, z])
    idx, sc, cnt = (t.cpu().numpy() for t in sim(m, [z]))
    assert np.array_equal(idx[0], np.delete(np.arange(N_ITEM), z)[:K]) and np.all(sc == 0.0) and cnt[0] == N_ITEM - 1      # all tie at 0: ascending ids
    osc = SO.sim_matrix(R["items"], R["coords"], 0.5, 5.0)[[z]]
    out = check(sim(m, [z], geo_weight=0.5, scale_km=5.0), osc, SO.candidate_mask([z], N_ITEM), K, "zero row by geo", min_ok=0.0)
    assert np.array_equal(out[0], SO.topk(osc, SO.candidate_mask([z], N_ITEM), K)[0]) and out[1].min() > 0.0


def test_twin_rows_stand_next_to_each_other_lower_id_first(pa):
    a, b = 41, 207                                            # (other tiles, other waves' quarters)
    R = SC.twin_case(a, b)
    m = model_of(pa, R, ("twin", a, b))
    osim = SO.sim_matrix(R["items"], R["coords"], 0.5, 5.0)
    assert np.array_equal(np.delete(osim[a], [a, b]), np.delete(osim[b], [a, b]))
    top = np.array([j for j in np.argsort(-osim[a]) if j not in (a, b)][:N_QUERY])      # the rows the twins are most similar to: they are on these lists
    try:
        for split_max, rows_max in ((SPLIT_MAX, 0), (0, 0), (SPLIT_MAX, 4096)):
            m.ctx.set_option("similar_split_max", split_max); m.ctx.set_option("similar_rows_max", rows_max)
            seen = 0
            for g, s in ((0.0, 1.0), (0.5, 5.0)):
                for k in (K, 32):
                    idx, sc, cnt = (t.cpu().numpy() for t in sim(m, top, k, geo_weight=g, scale_km=s))
                    for q in range(len(top)):
                        at = np.nonzero(idx[q] == a)[0]
                        if len(at) and at[0] + 1 < k:
                            assert idx[q, at[0] + 1] == b and bits(sc[q, at[0]]) == bits(sc[q, at[0] + 1]), (g, q)
                            seen += 1
                        assert not (idx[q] == b).any() or len(at), "the higher id is listed without the lower one"
            assert seen >= 4
            # the K-th and the (K + 1)-th entry tie: a list cut between the twins keeps the lower id
            full = sim(m, top, 32)[0].cpu().numpy()
            cut = [(q, int(np.nonzero(full[q] == a)[0][0])) for q in range(len(top)) if (full[q, :31] == a).any()]
            assert cut
            for q, at in cut[:4]:
                idx = sim(m, top[q:q + 1], at + 1)[0].cpu().numpy()
                assert idx[0, at] == a and not (idx[0] == b).any()
    finally:
        m.ctx.set_option("similar_split_max", SPLIT_MAX); m.ctx.set_option("similar_rows_max", ROWS_MAX)


# ---- 5: large k, half tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,s", [(0.0, 1.0), (0.5, 5.0)])
def test_large_k_goes_through_the_similarity_rows(pa, g, s):
    R = SC.poi_case("bpr", 20)
    m = model_of(pa, R, ("bpr", 20))
    pois = R["pois"]
    osc, mask = SC.sim_of("bpr", 20, g, s)[pois], SO.candidate_mask(pois, N_ITEM, *R["ex"])
    kw = dict(geo_weight=g, scale_km=s, exclude=R["ex"])
    fused = sim(m, pois, 32, **kw)
    for k in (33, 100, 299):
        out = sim(m, pois, k, **kw)
        idx, sc, cnt = check(out, osc, mask, k, "k %d g %g" % (k, g), min_ok=0.0)      # (with up to 300 gaps to clear few queries qualify)
        assert np.array_equal(idx[:, :32], fused[0].cpu().numpy()) and np.array_equal(bits(sc[:, :32]), bits(fused[1].cpu().numpy()))
        assert np.array_equal(cnt, fused[2].cpu().numpy())
        keep = m.SCORE_ROWS_BYTES
        try:
            m.SCORE_ROWS_BYTES = 4 * 320 * 16                 # 16 queries at a time: five chunks
            assert same(sim(m, pois, k, **kw), out), "chunked and unchunked buffers differ (k %d)" % k
        finally:
            m.SCORE_ROWS_BYTES = keep
    assert m.ctx.take_bad_ids() == 0


@pytest.mark.parametrize("kind,dim", SC.HALF_CASES)
def test_half_poi_table(pa, kind, dim):
    R = SC.half_case(kind, dim)
    m = model_of(pa, R, ("half", kind, dim))
    pois, x = R["pois"], m._diverse_items()
    assert x.dtype.itemsize == 2
    for g, s in GEO:
        osc = SC.sim_of(kind, dim, g, s, "half")[pois]
        out = fused(m, pois, geo_weight=g, scale_km=s, exclude=R["ex"])
        idx, sc, cnt = check(out, osc, SO.candidate_mask(pois, N_ITEM, *R["ex"]), K, "%s dim %d f16 g %g" % (kind, dim, g))
        assert same(sim(m, pois, geo_weight=g, scale_km=s, exclude=R["ex"]), out)
        rows = similar_rows(m, x, N_ITEM, pois, g, s)
        got = np.take_along_axis(rows, np.maximum(idx, 0), axis=1)
        assert np.array_equal(bits(sc)[idx >= 0], bits(got)[idx >= 0])


# ---- 6: the user side, and the models that are refused -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", SC.USER_CASES)
def test_similar_users(pa, kind, dim):
    import torch
    R = SC.user_case(kind, dim)
    m = model_of(pa, R, ("users", kind, dim))
    qs = R["qs"]
    su = lambda q, k=K, **kw: m.similar_users(q, k, return_scores=True, return_counts=True, **kw)
    ref = None
    for name, ex, mask in (("", None, SO.candidate_mask(qs, N_USER)), (", lists", R["ex"], SO.candidate_mask(qs, N_USER, *R["ex"]))):
        ref = check(su(qs, exclude=ex), R["sim"][qs], mask, K, "users %s dim %d%s" % (kind, dim, name))
        m.ctx.set_option("similar_rows_max", 0)               # ... and the fused walk
        try:
            assert same(su(qs, exclude=ex), tuple(torch.as_tensor(t) for t in ref))
        finally:
            m.ctx.set_option("similar_rows_max", ROWS_MAX)
    out = su(qs, 100, exclude=R["ex"])                        # the large-k route
    idx, sc, cnt = check(out, R["sim"][qs], SO.candidate_mask(qs, N_USER, *R["ex"]), 100, "users %s k 100" % kind, min_ok=0.0)
    assert np.array_equal(idx[:, :K], ref[0]) and np.array_equal(bits(sc[:, :K]), bits(ref[1])) and np.array_equal(cnt, ref[2])
    with pytest.raises(IndexError):
        m.similar_users([N_USER], K)
    assert m.ctx.take_bad_ids() == 0


def test_models_without_the_rows_refuse(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    m = _model(D.make_prme_synthetic(45, 700, 14, 4))
    assert not m._rank_fused and m._diverse_items() is None
    with pytest.raises(ValueError, match="users . items"):
        m.similar_users([0, 1], 5)
    with pytest.raises(ValueError, match="no single POI table"):
        m.similar_pois([0, 1], 5)
    with pytest.raises(ValueError, match="no single POI table"):
        m.nearest_visited([0, 1], [[3, 4], [5, 6]])


# ---- 7: the nearest visited POI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128)])
def test_nearest_visited(pa, kind, dim):
    N = SC.nearest_case(kind, dim)
    R = N["R"]
    m = model_of(pa, R, (kind, dim))
    n = R["C"]["T"]["n_user"]
    rows, lst = np.arange(n), N["lists"]
    for hist, arg in (("train", "train"), ("own", N["own"])):
        off, ids = N[hist]
        for g, s in ((0.0, 1.0), (0.5, 5.0), (1.0, 5.0)):
            pos, osim, gap, twin = SO.nearest(lst, off, ids, R["items"], R["coords"], g, s)
            poi, got = (t.cpu().numpy() for t in m.nearest_visited(rows, lst, histories=arg, geo_weight=g, scale_km=s, return_sims=True))
            want = np.where(pos >= 0, ids[np.minimum(off[:-1, None] + np.maximum(pos, 0), max(len(ids) - 1, 0))], -1)
            ok = (gap >= 1e-9) | twin
            assert ok[pos >= 0].mean() >= 0.9
            assert poi.dtype == np.int32 and np.array_equal(poi[ok], want[ok]), (hist, g)
            assert np.array_equal(poi < 0, pos < 0) and np.array_equal(np.isneginf(got), pos < 0)
            assert np.abs(got[pos >= 0] - osim[pos >= 0]).max() <= 1e-12, (hist, g)
    # a duplicated history POI resolves to its first position; an empty history and a -1 entry give -1
    off, ids = N["own"]
    x = m._diverse_items()
    import torch
    dev = lambda v, t=torch.int32: torch.as_tensor(np.asarray(v)).to(t).to(m.device)
    h = ids[off[2]:off[3]]
    assert h[0] == h[-1]
    l2 = np.full((1, K), -1, np.int64); l2[0, 0] = h[0]; l2[0, 3] = 5
    pos_t = torch.full((1, K), -7, dtype=torch.int32, device=m.device)
    sim_t = torch.zeros((1, K), dtype=torch.float64, device=m.device)
    l2_t, off_t, h_t = dev(l2), dev([0, len(h)]), dev(h)      # (kept alive across the call)
    m.ctx.check(m.lib.poi_similar_nearest(m.ctx.handle, vp(x), N_ITEM, x.shape[1], None, None, 0.0, 1.0, vp(l2_t), 1, K, vp(off_t), vp(h_t),
                                          vp(pos_t), vp(sim_t), m._stream()))
    p, sv = pos_t.cpu().numpy()[0], sim_t.cpu().numpy()[0]
    assert p[0] == 0 and abs(sv[0] - 1.0) <= 1e-12 and p[3] >= 0 and np.all(np.delete(p, [0, 3]) == -1) and np.all(np.isneginf(np.delete(sv, [0, 3])))
    empty = m.nearest_visited([4], lst[4:5], histories=(np.array([0, 0]), np.zeros(0, np.int64)))
    assert np.all(empty.cpu().numpy() == -1)
    # a row alone against the same row in the call
    whole = m.nearest_visited(rows, lst, geo_weight=0.5, scale_km=5.0, return_sims=True)
    for r in (0, 7, 33, n - 1):
        alone = m.nearest_visited([r], lst[r:r + 1], geo_weight=0.5, scale_km=5.0, return_sims=True)
        assert all(np.array_equal(a.cpu().numpy().view(np.int32), b[r:r + 1].cpu().numpy().view(np.int32)) for a, b in zip(alone, whole)), r
    pick = np.array([5, 2, 40])                               # (not a contiguous range: the histories are gathered)
    some = m.nearest_visited(pick, lst[pick], geo_weight=0.5, scale_km=5.0, return_sims=True)
    assert all(np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy()[pick].view(np.int32)) for a, b in zip(some, whole))
    # ids outside the table: host arrays raise, device tensors reject the row, counted once
    with pytest.raises(IndexError):
        m.nearest_visited([0], [[N_ITEM]])
    with pytest.raises(IndexError):
        m.nearest_visited([0], [[3]], histories=([0, 1], [N_ITEM]))
    bad = lst[:3].copy(); bad[1, 2] = N_ITEM
    clean = m.nearest_visited(rows[:3], lst[:3]).cpu().numpy()
    out = m.nearest_visited(rows[:3], dev(bad), sync=False).cpu().numpy()
    assert m.ctx.take_bad_ids() == 1 and np.all(out[1] == -1) and np.array_equal(out[[0, 2]], clean[[0, 2]])
    hb = ids[:off[3]].copy(); hb[off[1]] = N_ITEM
    clean = m.nearest_visited(rows[:3], lst[:3], histories=(off[:4], ids[:off[3]])).cpu().numpy()
    out = m.nearest_visited(rows[:3], lst[:3], histories=(dev(off[:4]), dev(hb)), sync=False).cpu().numpy()
    assert m.ctx.take_bad_ids() == 1 and np.all(out[1] == -1) and np.array_equal(out[[0, 2]], clean[[0, 2]])
    with pytest.raises(IndexError):
        m.nearest_visited(rows[:3], dev(bad))
