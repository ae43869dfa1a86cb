"""-m gpu tests of the audience recommendation (poi_score_audience / poi_audience_rows -> models.recommend_audience, Session.audience,
evaluate.audience_recall): given a POI, which users?  The ranking contract against the float64 oracle of tests/audience_oracle.py (the
score matrix of tests/near_oracle.py, transposed) on the cases of tests/audience_cases.py, the bits against poi_score_rows, both launch
regimes on every grid, invariance, tiny tables, ties, the large-k route, half tables, the models that rank by their own score rows,
sessions, segments, the evaluation and the contract."""
import ctypes

import numpy as np
import pytest

from tests import audience_cases as AC
from tests import audience_oracle as AO
from tests.audience_cases import K, N_ITEM, N_QUERY, N_USER
from tests.test_gpu_near import built, check

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("audience_path", "audience_splits", "audience_split_max")
SPLIT_MAX = 256                                      # the option's default


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


_MODELS = {}


def model_of(pa, R, key):
    """(model, oracle scores (n_item, n)) of a case, built once per module: on the spatial case the rows of NO_LAST lose their last POI in
    the scoring snapshot; VBPR's item table is formed on the device, so its oracle reads that float32 table."""
    if key not in _MODELS:
        C = R["C"]
        m, items = built(pa, C)
        if C["kind"] == "spatial":
            m._last_poi[[r for r in AC.NO_LAST if r < C["T"]["n_user"]]] = -1
        sct = R["sct"] if items is None else AO.scores_t(C["users"], items, R["last"], C["term"], C["T"])
        _MODELS[key] = (m, sct)
    return _MODELS[key]


def rank_model(pa, kind, dim, n_user=N_USER):
    return model_of(pa, AC.rank_case(kind, dim, n_user), (kind, dim, n_user))


def aud(m, pois, k=K, **kw):
    return m.recommend_audience(pois, k, return_scores=True, return_counts=True, **kw)


def same(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32)) for x, y in zip(a, b))


def operands(m):
    """(users rows, term, the 13 leading arguments) of every user, as recommend_audience assembles them."""
    ids, users, lo = m._users_rows(np.arange(m.n_user))
    term = m._rank_term(ids, lo)
    return users.contiguous(), term, m._tile_operands(users.contiguous(), m._items(), m.kdim, term)


def score_rows(m):
    """poi_score_rows of every user: (n_user, n_item) float32."""
    import torch
    users, term, ops = operands(m)
    out = torch.empty((m.n_user, m.n_item), dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_score_rows(m.ctx.handle, *ops, ctypes.c_void_p(out.data_ptr()), m.n_item, m._stream()))
    return out.cpu().numpy()


def audience_rows(m, pois, ld=None):
    """poi_audience_rows of the queries: (n_q, ld) float32, NaN where the kernel wrote nothing."""
    import torch
    users, term, ops = operands(m)
    ld = ld or m.n_user
    q = torch.as_tensor(np.asarray(pois, np.int32)).to(m.device)
    out = torch.full((len(pois), ld), float("nan"), dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_audience_rows(m.ctx.handle, *ops, ctypes.c_void_p(q.data_ptr()), len(pois), ctypes.c_void_p(out.data_ptr()), ld, m._stream()))
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1: ranking and bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", AC.RANK_CASES)
def test_ranking_matches_the_oracle_and_the_bits_of_score_rows(pa, kind, dim):
    R = AC.rank_case(kind, dim)
    m, sct = rank_model(pa, kind, dim)
    pois = R["pois"]
    osc = sct[pois]
    full = score_rows(m)                                      # (n_user, n_item): what poi_score_rank / poi_score_rows compute
    for name, ex, mask in (("", None, AO.candidate_mask(N_QUERY, N_USER)), (", train visitors", "train", AO.candidate_mask(N_QUERY, N_USER, *R["vis"]))):
        idx, sc, cnt = check(aud(m, pois, exclude=ex), osc, mask, K, "%s dim %d%s" % (kind, dim, name))
        g = np.maximum(idx, 0)
        want = full[g, pois[:, None]]
        assert np.array_equal(bits(sc)[idx >= 0], bits(want)[idx >= 0]), "score_out differs from poi_score_rows in some bit"
    rows = audience_rows(m, pois, ld=N_USER + 3)
    assert np.array_equal(bits(rows[:, :N_USER]), bits(full[:, pois].T)) and np.isnan(rows[:, N_USER:]).all()
    assert m.ctx.take_bad_ids() == 0


# ---- 2: regimes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 32)])
def test_every_grid_and_both_regimes_give_the_same_bits(pa, kind, dim):
    n_user = 3001                                             # 94 user tiles: 64 slices are not empty
    R = AC.rank_case(kind, dim, n_user)
    m, sct = rank_model(pa, kind, dim, n_user)
    pois = R["pois"]
    plan = lambda: {k: m.ctx.last_plan(k) for k in PLAN_KEYS}
    try:
        ref = aud(m, pois, exclude="train")                   # 70 queries: the split regime, slices by the CUs
        p = plan()
        assert p["audience_path"] == 1 and 1 <= p["audience_splits"] <= 64 and p["audience_split_max"] == SPLIT_MAX, p
        check(ref, sct[pois], AO.candidate_mask(N_QUERY, n_user, *R["vis"]), K, "%s default plan" % kind)
        rows = audience_rows(m, pois)
        for grid in (1, 2, 3, 7, 64):
            m.ctx.set_option("audience_split_max", 1 << 30); m.ctx.set_option("audience_grid", grid)
            out = aud(m, pois, exclude="train")
            assert plan() == dict(audience_path=1, audience_splits=grid, audience_split_max=1 << 30)
            assert same(out, ref), "grid %d differs" % grid
            assert np.array_equal(bits(audience_rows(m, pois)), bits(rows)), "rows: grid %d differs" % grid
        m.ctx.set_option("audience_split_max", 0); m.ctx.set_option("audience_grid", 0)
        out = aud(m, pois, exclude="train")
        assert plan() == dict(audience_path=0, audience_splits=0, audience_split_max=0)
        assert same(out, ref), "one workgroup per query block differs from the slices"
        assert np.array_equal(bits(audience_rows(m, pois)), bits(rows))
    finally:
        m.ctx.set_option("audience_split_max", SPLIT_MAX); m.ctx.set_option("audience_grid", 0)


# ---- 3: invariance ---------------------------------------------------------------------------------------------------------------------
def test_a_query_does_not_depend_on_its_call(pa):
    R = AC.rank_case("spatial", 32)
    m, sct = rank_model(pa, "spatial", 32)
    pois = R["pois"]
    ref = aud(m, pois, exclude="train")
    for q in (0, 1, 31, 32, 63, 64, 69):                      # alone against the same query inside the call of 70
        assert same(aud(m, pois[q:q + 1], exclude="train"), tuple(t[q:q + 1] for t in ref)), "query %d alone differs" % q
    try:
        for split_max in (SPLIT_MAX, 0):
            m.ctx.set_option("audience_split_max", split_max)
            for n_q in (1, 31, 32, 33):
                assert same(aud(m, pois[:n_q], exclude="train"), tuple(t[:n_q] for t in ref)), "the first %d queries differ" % n_q
            twice = np.array([pois[5], pois[40], pois[5]])
            out = aud(m, twice, exclude="train")
            assert same(tuple(t[0:1] for t in out), tuple(t[2:3] for t in out)) and same(tuple(t[0:1] for t in out), tuple(t[5:6] for t in ref))
    finally:
        m.ctx.set_option("audience_split_max", SPLIT_MAX)


# ---- 4: tiny tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_user", [6, 13])
def test_tiny_user_tables_fill_and_count(pa, n_user):
    R = AC.rank_case("bpr", 20, n_user)
    m, sct = rank_model(pa, "bpr", 20, n_user)
    pois = R["pois"]
    idx, sc, cnt = check(aud(m, pois), sct[pois], AO.candidate_mask(N_QUERY, n_user), K, "%d users" % n_user)
    assert np.all(cnt == n_user) and np.all(idx[:, n_user:] == -1) and np.all(idx[:, :n_user] >= 0)
    check(aud(m, pois, exclude="train"), sct[pois], AO.candidate_mask(N_QUERY, n_user, *R["vis"]), K, "%d users, train visitors" % n_user)
    everyone = (np.arange(4) * n_user, np.tile(np.arange(n_user), 3))      # three queries whose lists exclude everyone
    idx, sc, cnt = (t.cpu().numpy() for t in aud(m, pois[:3], exclude=everyone))
    assert np.all(cnt == 0) and np.all(idx == -1) and np.all(np.isneginf(sc))
    assert m.ctx.take_bad_ids() == 0


# ---- 5: ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bpr", "gru"])
def test_twin_users_stand_next_to_each_other_lower_id_first(pa, kind):
    a, b = 211, 900                                           # (other tiles, other waves' quarters)
    R = AC.twin_case(kind, a, b)
    m, sct = model_of(pa, R, ("twin", kind))
    assert np.array_equal(sct[:, a], sct[:, b])
    top = np.argsort(-sct[:, a])[:N_QUERY]                    # the POIs the twins like best: they are on these lists
    try:
        for split_max in (SPLIT_MAX, 0):
            m.ctx.set_option("audience_split_max", split_max)
            seen = 0
            for k in (K, 32):
                idx, sc, cnt = (t.cpu().numpy() for t in aud(m, top, k))
                for q in range(len(top)):
                    at = np.nonzero(idx[q] == a)[0]
                    if len(at) and at[0] + 1 < k:
                        assert idx[q, at[0] + 1] == b and bits(sc[q, at[0]]) == bits(sc[q, at[0] + 1]), (kind, q)
                        seen += 1
                    assert not (idx[q] == b).any() or len(at), "the higher id is listed without the lower one"
            assert seen >= 4
            # the K-th and the (K + 1)-th entry tie: a list cut between the twins keeps the lower id
            full = aud(m, top, 32)[0].cpu().numpy()
            cut = [(q, int(np.nonzero(full[q] == a)[0][0])) for q in range(len(top)) if (full[q, :31] == a).any()]
            assert cut
            for q, at in cut[:6]:
                idx = aud(m, top[q:q + 1], at + 1)[0].cpu().numpy()
                assert idx[0, at] == a and not (idx[0] == b).any()
    finally:
        m.ctx.set_option("audience_split_max", SPLIT_MAX)


# ---- 6: large k ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 32)])
def test_large_k_goes_through_the_score_rows(pa, kind, dim):
    R = AC.rank_case(kind, dim)
    m, sct = rank_model(pa, kind, dim)
    pois = R["pois"]
    osc, mask = sct[pois], AO.candidate_mask(N_QUERY, N_USER, *R["vis"])
    fused = aud(m, pois, 32, exclude="train")
    for k in (33, 100, 1000):
        out = aud(m, pois, k, exclude="train")
        # (exact on the qualifying queries; with 1001 gaps to clear few queries qualify, so the share is not held to check's 90 % here -
        # every other property of the contract holds on every query)
        assert AO.qualifying(osc, mask, k).any()
        idx, sc, cnt = check(out, osc, mask, k, "%s k %d" % (kind, k), min_ok=0.0)
        assert np.array_equal(idx[:, :32], fused[0].cpu().numpy()) and np.array_equal(bits(sc[:, :32]), bits(fused[1].cpu().numpy()))
        assert np.array_equal(cnt, fused[2].cpu().numpy())
        keep = m.SCORE_ROWS_BYTES
        try:
            m.SCORE_ROWS_BYTES = 4 * 1056 * 16                # 16 queries at a time: five chunks
            assert same(aud(m, pois, k, exclude="train"), out), "chunked and unchunked buffers differ (k %d)" % k
        finally:
            m.SCORE_ROWS_BYTES = keep
    assert m.ctx.take_bad_ids() == 0


# ---- 7: half tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", AC.HALF_CASES)
def test_half_poi_table(pa, kind, dim):
    R = AC.half_case(kind, dim)
    m, sct = model_of(pa, R, ("half", kind, dim))
    pois = R["pois"]
    for ex, mask in ((None, AO.candidate_mask(N_QUERY, N_USER)), ("train", AO.candidate_mask(N_QUERY, N_USER, *R["vis"]))):
        check(aud(m, pois, exclude=ex), sct[pois], mask, K, "%s dim %d f16" % (kind, dim))
    full = score_rows(m)
    assert np.array_equal(bits(audience_rows(m, pois)), bits(full[:, pois].T))


# ---- 8: the models that rank by a rule of their own -----------------------------------------------------------------------------------
def own_rows_check(m, full, what, train=True, k=K, min_ok=0.9):
    """full: (n_user, n_item) float64, the model's own score rows.  Every query, lists of user ids, a segment; with `train` the model's
    own train visitors (it keeps an (off, p) train table).  The oracle reads the very float32 rows the selection reads, so beyond the
    contract every list is the oracle's to the id, ties included (min_ok: the share of queries `check` wants without a near-tie - the
    CA-RNN toy problem has users with equal states, whose scores tie exactly)."""
    def check_exact(out, osc, mask, k, what):
        idx = check(out, osc, mask, k, what, min_ok=min_ok)[0]
        assert np.array_equal(idx, AO.topk(osc, mask, k)[0]), what
    import torch
    n_user, n_item = full.shape
    pois = AC.queries(31, min(40, n_item), n_item)
    osc = full.T[pois]
    k = min(k, n_user)
    rng = np.random.default_rng(41)
    ex = AO.csr([np.sort(rng.choice(n_user, rng.integers(0, n_user // 2), replace=False)) for _ in pois])
    check_exact(aud(m, pois, k), osc, AO.candidate_mask(len(pois), n_user), k, what)
    check_exact(aud(m, pois, k, exclude=ex), osc, AO.candidate_mask(len(pois), n_user, *ex), k, what + ", lists")
    seg = np.arange(1, n_user, 2)
    ks = min(k, len(seg))
    pos = {int(u): i for i, u in enumerate(seg)}
    exs = AO.csr([[pos[int(u)] for u in ex[1][a:b] if int(u) in pos] for a, b in zip(ex[0][:-1], ex[0][1:])])
    out = aud(m, pois, ks, users=seg, exclude=ex)
    idx = out[0].cpu().numpy()
    assert np.all((idx < 0) | np.isin(idx, seg))
    back = np.where(idx >= 0, np.searchsorted(seg, np.maximum(idx, 0)), -1).astype(np.int32)
    check_exact((torch.as_tensor(back), out[1], out[2]), osc[:, seg], AO.candidate_mask(len(pois), len(seg), *exs), ks, what + ", segment")
    if train:
        off, p = m._off_host.astype(np.int64), m.p.cpu().numpy()
        vis = AO.visitor_lists([p[a:b] for a, b in zip(off[:-1], off[1:])], n_item, pois)
        check_exact(aud(m, pois, k, exclude="train"), osc, AO.candidate_mask(len(pois), n_user, *vis), k, what + ", train visitors")
    else:
        with pytest.raises(Exception, match="train table"):
            aud(m, pois, k, exclude="train")
    assert m.ctx.take_bad_ids() == 0


def test_scores_route_through_prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(45, 700, 14, 4)
    m = _model(ds)
    m.update_trained_items()
    full = m.compute_sub_all_scores(np.arange(ds.n_user))
    own_rows_check(m, np.float64(full.reshape(ds.n_user, -1, ds.n_item)[:, 0]), "prme")


def test_scores_route_through_poi2vec(pa):
    from poi_amd import data as D, harness
    ds = D.make_poi2vec_synthetic(60, 200, 12, 13, local=0.9, n_nbr=8)
    m = harness.poi2vec_model(ds, dict(latent_size=20, seed=5, softmax_axis="items", eval_context="test"))
    m.update_trained_params()
    full = m.compute_sub_all_scores(np.arange(60))
    own_rows_check(m, np.float64(full.reshape(60, -1, m.n_item)[:, 0]), "poi2vec", train=False)


def test_scores_route_through_carnn_and_its_session_is_refused(pa):
    from tests.test_gpu_group import carnn_model
    m = carnn_model(pa)
    own_rows_check(m, np.float64(m.compute_sub_all_scores(np.arange(21))), "carnn", min_ok=0.0)
    with pytest.raises(pa._lib.PoiError, match="OboCARNN"):
        m.cell_session().audience([0, 1], 5)


# ---- 9: sessions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "lstm"])
def test_session_audience(pa, kind):
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    n_slot = T["n_user"] + 1
    if kind == "spatial":
        P = TS.spatial_init(32, T)
        s = TS.spatial_model(pa, T, P).session(n_slot=n_slot)
    else:
        P = TC.params("lstm", 60, T)
        s = TC.model(pa, "lstm", T, P).cell_session(n_slot=n_slot)
    for t in range(3):                                       # three check-ins per slot; the last slot never checks in
        s.advance(np.arange(T["n_user"]), T["train"][0][:, t])
    st = s.state()
    users = np.float64(np.float32(st["h"]))                  # the kernel reads the float32 rounding of the state
    term = (float(P["wd"]), np.float64(st["sts"])) if kind == "spatial" else None
    assert st["last_poi"][-1] == -1
    sct = AO.scores_t(users, P["lt"], st["last_poi"], term, T)
    pois = AC.queries(17, 40, T["n_item"])
    rng = np.random.default_rng(3)
    ex = AO.csr([np.sort(rng.choice(n_slot, rng.integers(0, 30), replace=False)) for _ in pois])
    out = s.audience(pois, K, exclude=ex, return_scores=True, return_counts=True)
    check(out, sct[pois], AO.candidate_mask(len(pois), n_slot, *ex), K, "session %s" % kind)
    seg = np.arange(0, n_slot, 3)
    idx = s.audience(pois, 10, slots=seg).cpu().numpy()
    oid = AO.topk(sct[pois][:, seg], AO.candidate_mask(len(pois), len(seg)), 10)[0]
    ok = AO.qualifying(sct[pois][:, seg], AO.candidate_mask(len(pois), len(seg)), 10)
    assert ok.mean() >= 0.9 and np.array_equal(idx[ok], seg[oid[ok]])
    with pytest.raises(IndexError):
        s.audience([T["n_item"]], K)
    with pytest.raises(ValueError):
        s.audience(pois, K, exclude="train")


# ---- 10: segments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 32), ("fpmc", 20)])
def test_a_segment_of_users(pa, kind, dim):
    import torch
    R = AC.rank_case(kind, dim)
    m, sct = rank_model(pa, kind, dim)
    pois = R["pois"]
    seg = np.sort(np.random.default_rng(8).choice(N_USER, 400, replace=False))
    seg[-1] = N_USER - 1
    seg = np.unique(seg)
    from tests.test_gpu_session import seqs_of
    vs = AO.visitor_lists(seqs_of(R["C"]["T"]), N_ITEM, pois, seg)
    for ex, mask in ((None, AO.candidate_mask(N_QUERY, len(seg))), ("train", AO.candidate_mask(N_QUERY, len(seg), *vs))):
        out = aud(m, pois, users=seg, exclude=ex)
        idx = out[0].cpu().numpy()
        assert np.all((idx < 0) | np.isin(idx, seg)), "the ids returned are user ids of the segment"
        back = np.where(idx >= 0, np.searchsorted(seg, np.maximum(idx, 0)), -1).astype(np.int32)
        check((torch.as_tensor(back), out[1], out[2]), sct[pois][:, seg], mask, K, "%s segment %s" % (kind, ex))
    # a CSR pair of user ids, restricted to the segment on the way
    off, ids = R["vis"]
    a = aud(m, pois, users=seg, exclude=(off, ids))
    assert same(a, aud(m, pois, users=seg, exclude="train"))


# ---- 11: evaluation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [None, "train"])
def test_audience_recall_equals_the_host_number(pa, exclude):
    from poi_amd import evaluate
    from tests.test_gpu_session import seqs_of
    R = AC.rank_case("bpr", 20)
    m, sct = rank_model(pa, "bpr", 20)
    T = R["C"]["T"]
    ks = [5, 20, 100]
    got = evaluate.audience_recall(m, ks, exclude=exclude)
    tes = np.asarray(T["test"][0]).reshape(N_USER, -1)
    vis = AO.visitor_sets(seqs_of(T), N_ITEM)
    lim = 1e-5 * np.abs(sct).max()                            # the margin a float32 score is held within (tests/gpu_util.RTOL)
    sure, maybe, total = np.zeros(len(ks)), np.zeros(len(ks)), 0
    for u in range(N_USER):
        for j in tes[u]:
            if exclude == "train" and u in vis[j]:
                continue                                      # the pair is no candidate: it leaves the mean
            cand = np.ones(N_USER, bool)
            if exclude == "train":
                cand[sorted(vis[j])] = False
            s = sct[j, cand]
            lo, hi = int((s > sct[j, u] + lim).sum()), int((s >= sct[j, u] - lim).sum()) - 1      # the rank lies in [lo, hi]
            total += 1
            sure += [hi < k for k in ks]
            maybe += [lo < k <= hi for k in ks]
    print("audience recall", exclude, got, sure / total, "pairs within the margin of a cut-off:", maybe)
    assert total > 0 and maybe.max() <= 0.02 * total
    for i, k in enumerate(ks):
        assert sure[i] - 1e-9 <= got[k] * total <= sure[i] + maybe[i] + 1e-9, (k, got[k], sure[i] / total)


# ---- 12: contract ----------------------------------------------------------------------------------------------------------------------
def test_contract(pa):
    import torch
    R = AC.rank_case("bpr", 20)
    m, sct = rank_model(pa, "bpr", 20)
    pois = R["pois"]
    dev = lambda v: torch.as_tensor(np.asarray(v, np.int32)).to(m.device)
    clean = tuple(t.cpu().numpy() for t in aud(m, pois[:8], exclude="train"))
    # host ids out of range raise before the launch
    for bad in ([N_ITEM], [-1], [3, N_ITEM + 5]):
        with pytest.raises(IndexError):
            m.recommend_audience(bad, K)
    with pytest.raises(IndexError):
        m.recommend_audience(pois, K, users=[0, N_USER])
    with pytest.raises(ValueError):
        m.recommend_audience(pois, K, users=[5, 3])
    with pytest.raises(ValueError):
        m.recommend_audience(pois, K, users=[3, 3])
    with pytest.raises(IndexError):
        m.recommend_audience(pois[:2], K, exclude=([0, 1, 2], [0, N_USER]))
    with pytest.raises(ValueError):
        m.recommend_audience(pois[:2], K, exclude=([0, 2, 4], [5, 3, 1, 2]))
    with pytest.raises(ValueError):
        m.recommend_audience(pois, K, exclude="last")
    for k in (0, N_USER + 1, 5000):
        with pytest.raises(ValueError):
            m.recommend_audience(pois, k)
    assert m.ctx.take_bad_ids() == 0
    # device tensors: a bad query id is the kernel's to find
    q = pois[:8].copy(); q[5] = N_ITEM
    with pytest.raises(IndexError):
        m.recommend_audience(dev(q), K, exclude="train")
    for k in (K, 40):                                        # the fused walk, and the score rows + selection
        ref = tuple(t.cpu().numpy() for t in aud(m, pois[:8], k, exclude="train"))
        idx, sc, cnt = (t.cpu().numpy() for t in aud(m, dev(q), k, exclude="train", sync=False))
        assert m.ctx.take_bad_ids() == 1
        assert np.all(idx[5] == -1) and np.all(np.isneginf(sc[5])) and cnt[5] == 0
        good = np.arange(8) != 5
        assert all(np.array_equal(x[good], y[good]) for x, y in zip((idx, sc, cnt), ref)), "the other queries changed"
    # ... and so is a broken list: not ascending / a row outside [0, n)
    off, ids = (np.asarray(v)[:9 if i == 0 else None] for i, v in enumerate(R["vis"]))
    ids = ids[:off[-1]]
    assert off[3] - off[2] >= 2
    for breaker in (lambda e: e.__setitem__(off[2] + 1, e[off[2]]), lambda e: e.__setitem__(off[3] - 1, N_USER)):
        e = ids.copy(); breaker(e)
        idx, sc, cnt = (t.cpu().numpy() for t in aud(m, dev(pois[:8]), exclude=(dev(off), dev(e)), sync=False))
        assert m.ctx.take_bad_ids() == 1
        assert np.all(idx[2] == -1) and np.all(np.isneginf(sc[2])) and cnt[2] == 0
        good = np.arange(8) != 2
        assert all(np.array_equal(x[good], y[good]) for x, y in zip((idx, sc, cnt), clean))
        with pytest.raises(IndexError):
            aud(m, dev(pois[:8]), exclude=(dev(off), dev(e)))
    # poi_audience_rows: the row of a rejected query is -inf, counted once
    rows = audience_rows(m, q)
    assert m.ctx.take_bad_ids() == 1 and np.all(np.isneginf(rows[5])) and np.isfinite(np.delete(rows, 5, axis=0)).all()
    # the C entry: k = 33 is not supported
    users, term, ops = operands(m)
    out = torch.empty((8, 33), dtype=torch.int32, device=m.device)
    rc = m.lib.poi_score_audience(m.ctx.handle, *ops, ctypes.c_void_p(dev(pois[:8]).data_ptr()), 8, None, None, 33, ctypes.c_void_p(out.data_ptr()),
                                  None, None, m._stream())
    assert rc == -4                                           # POI_ENOTSUP
    with pytest.raises(pa._lib.PoiError, match="k <= 32"):
        m.ctx.check(rc)
    assert m.ctx.take_bad_ids() == 0
