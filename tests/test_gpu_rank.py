"""-m gpu tests of the exact target rank (poi_score_rank / poi_rank_scores, models.compute_sub_target_rank, Session.rank_of,
evaluate.full_rank_metrics) against the float64 oracle of tests/rank_oracle.py, run on the float32-rounded user rows and tables.

The bar: where no other POI's float64 score lies within 1e-6 max|score of the row| of the target's (a == 0, the gap rule of
tests/test_gpu_fullsize.py) the rank is exact; otherwise it lies in [greater_clear, greater_clear + a].  At least 95 % of the valid
(row, target) pairs must have a == 0 - asserted on the oracle alone.  Identities of the code's own paths (a target taken from the
model's own top-K list sits at that position; poi_rank_scores equals a host count over the same matrix) are exact everywhere."""
import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import rank_oracle as RO
from tests.gpu_util import RTOL, round_f32, toy_problem
from tests.test_gpu_session import K, geo_problem, gru_init, oracle_scores, plain_model, qualifying, spatial_init, spatial_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


# ---- problems ----------------------------------------------------------------------------------------------------------------------
def rows_of(seed, T, spatial):
    """float32-rounded user rows (and bin probabilities) that stand for a trained model's: what both sides rank with."""
    rng = np.random.default_rng(seed + 77)
    hts = rng.uniform(-0.5, 0.5, (T["n_user"], T["dim"])).astype(np.float32).astype(np.float64)
    sts = rng.uniform(0.0, 1.0, (T["n_user"], T["n_dist"] + 1)).astype(np.float32).astype(np.float64) if spatial else None
    return hts, sts


def targets_of(seed, T, len_t):
    """(tgt, mask): len_t targets per row, distinct within a row, ragged masks for len_t > 1 (position 0 always valid)."""
    rng = np.random.default_rng(seed + 99)
    n, N = T["n_user"], T["n_item"]
    tgt = np.stack([rng.choice(N, len_t, replace=False) for _ in range(n)]).astype(np.int32)
    tm = np.ones((n, len_t), np.int32)
    if len_t > 1:
        tm[:, 1:] = rng.random((n, len_t - 1)) < 0.6
    return tgt, tm


def build(pa, seed, n, n_item, dim, spatial, cls="OboGru", **kw):
    import torch
    T = geo_problem(seed, n_user=n, n_item=n_item, n_dist=11, dim=dim, len_min=4, len_max=8)
    P = spatial_init(seed, T) if spatial else gru_init(seed, T)
    hts, sts = rows_of(seed, T, spatial)
    if cls == "OboBpr":
        m = plain_model(pa, T, dict(ux=hts, lt=P["lt"]), cls, **kw)
        m.update_trained_users()
    else:
        m = spatial_model(pa, T, P, **kw) if spatial else plain_model(pa, T, P, cls, **kw)
        m.update_trained_users(torch.as_tensor(hts))
        if spatial:
            m.update_trained_sus(torch.as_tensor(sts))
    last = [T["train"][0][u, L - 1] for u, L in enumerate(T["lens"])]
    return T, P, m, hts, sts, last


def check_against_oracle(got, orc, what=""):
    got = np.asarray(got, np.int64)
    valid = orc["rank"] >= 0
    assert np.array_equal(got >= 0, valid), what + ": the ranked positions differ"
    share = (orc["a"][valid] == 0).mean() if valid.any() else 1.0
    print("%s: %d pairs, a == 0 for %.2f %%, max a %d" % (what, valid.sum(), 100 * share, orc["a"].max()))
    assert share >= 0.95, "%s: only %.1f %% of the oracle's pairs have a clear gap" % (what, 100 * share)
    exact = valid & (orc["a"] == 0)
    assert np.array_equal(got[exact], orc["rank"][exact]), what + ": rank differs where the gap is clear"
    loose = valid & (orc["a"] > 0)
    lo, hi = orc["greater_clear"][loose], (orc["greater_clear"] + orc["a"])[loose]
    assert ((got[loose] >= lo) & (got[loose] <= hi)).all(), what + ": rank outside the band's bounds"


# ---- the fused entry against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_item,n,dim,len_t,spatial", [
    (31, 31, 8, 1, False), (32, 31, 20, 3, True), (33, 33, 64, 1, True), (50, 70, 128, 3, False), (300, 33, 64, 3, True),
    (300, 1, 20, 1, True), (2049, 70, 128, 1, True), (2049, 31, 8, 3, False), (2049, 33, 20, 3, True), (50, 31, 64, 1, False),
    (200, 33, 160, 1, True)])        # (the fourth dim bracket, 129 .. 256: one full row tile and a row, six item tiles and a tail)
def test_rank_matches_the_oracle(pa, n_item, n, dim, len_t, spatial):
    seed = 7 * n_item + n + dim
    T, P, m, hts, sts, last = build(pa, seed, n, n_item, dim, spatial)
    sc = oracle_scores(P, T, hts, sts, last)
    tgt, tm = targets_of(seed, T, len_t)
    orc = RO.ranks(sc, tgt, tm)
    rank, val, cnt = m.compute_sub_target_rank(np.arange(n), targets=(tgt, tm), return_scores=True, return_counts=True)
    assert rank.dtype.is_floating_point is False and tuple(rank.shape) == (n, len_t)
    check_against_oracle(rank.cpu().numpy(), orc, "n_item %d n %d dim %d len_t %d %s" % (n_item, n, dim, len_t, "spatial" if spatial else "plain"))
    assert np.array_equal(cnt.cpu().numpy(), orc["count"])
    v, ok = val.cpu().numpy(), orc["rank"] >= 0
    assert np.all(np.abs(v[ok] - orc["score"][ok]) <= RTOL * np.abs(sc).max()) and np.isneginf(v[~ok]).all()


def test_rank_default_targets_bpr_and_id_lists(pa):
    T, P, m, hts, sts, last = build(pa, 501, 70, 300, 64, False, cls="OboBpr")
    sc = O.score_all(hts, P["lt"])
    tes = T["test"][0]
    orc = RO.ranks(sc, tes, np.ones_like(tes))
    check_against_oracle(m.compute_sub_target_rank(np.arange(70)).cpu().numpy(), orc, "OboBpr")
    ids = np.array([9, 3, 60, 17])
    check_against_oracle(m.compute_sub_target_rank(ids).cpu().numpy(), {k: v[ids] for k, v in orc.items()}, "OboBpr id list")


def test_rank_on_a_registered_half_table(pa):
    T, P, m, hts, sts, last = build(pa, 502, 33, 300, 64, False, table_dtype="f16")
    Ph = dict(P, lt=P["lt"].astype(np.float16).astype(np.float64))
    sc = O.score_all(hts, Ph["lt"])
    tgt, tm = targets_of(502, T, 3)
    check_against_oracle(m.compute_sub_target_rank(np.arange(33), targets=(tgt, tm)).cpu().numpy(), RO.ranks(sc, tgt, tm), "half table")


# ---- exclusion ------------------------------------------------------------------------------------------------------------------------
def test_exclusion_lists(pa):
    import torch
    n, N = 33, 300
    T, P, m, hts, sts, last = build(pa, 503, n, N, 64, True)
    sc = oracle_scores(P, T, hts, sts, last)
    tgt, tm = targets_of(503, T, 3)
    # the users' train POIs
    eo, ex = (t.cpu().numpy() for t in m.train_exclusion())
    orc = RO.ranks(sc, tgt, tm, eo, ex)
    rank, cnt = m.compute_sub_target_rank(np.arange(n), exclude="train", targets=(tgt, tm), return_counts=True)
    check_against_oracle(rank.cpu().numpy(), orc, "train exclusion")
    assert np.array_equal(cnt.cpu().numpy(), orc["count"]) and (orc["count"] < N).all()
    # empty lists; a list holding the target; a list holding every POI but the target
    t0 = tgt[:, 0]
    off = np.zeros(n + 1, np.int32); ids = np.zeros(0, np.int32)
    lists = []
    for r in range(n):
        lists.append(np.zeros(0, np.int32) if r % 3 == 0 else np.array([t0[r]], np.int32) if r % 3 == 1 else np.delete(np.arange(N, dtype=np.int32), t0[r]))
    off[1:] = np.cumsum([len(l) for l in lists]); ids = np.concatenate(lists).astype(np.int32)
    one = (tgt[:, :1].copy(), np.ones((n, 1), np.int32))
    orc = RO.ranks(sc, one[0], one[1], off, ids)
    rank, cnt = m.compute_sub_target_rank(np.arange(n), exclude=(off, ids), targets=one, return_counts=True)
    rank, cnt = rank.cpu().numpy()[:, 0], cnt.cpu().numpy()
    check_against_oracle(rank[:, None], orc, "hand-made exclusion")
    assert (rank[1::3] == -1).all() and (rank[2::3] == 0).all() and (cnt[2::3] == 1).all() and (cnt[0::3] == N).all() and (cnt[1::3] == N - 1).all()
    # device lists go unchecked on the host and give the same
    r2 = m.compute_sub_target_rank(np.arange(n), exclude=(torch.as_tensor(off).to(m.device), torch.as_tensor(ids).to(m.device)), targets=one)
    assert np.array_equal(r2.cpu().numpy()[:, 0], rank)


# ---- planted ties ---------------------------------------------------------------------------------------------------------------------
def raw_rank(m, users, items, tgt, tm, n_item, dim):
    import torch
    from poi_amd.models import _ptr
    n, lt = tgt.shape
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(m.device)
    u, it, t, k = dev(users, torch.float32), dev(items, torch.float32), dev(tgt, torch.int32), dev(tm, torch.int32)
    rank = torch.empty((n, lt), dtype=torch.int32, device=m.device)
    m.ctx.check(m.lib.poi_score_rank(m.ctx.handle, _ptr(u), _ptr(it), n, n_item, dim, None, None, None, None, None, None, 0, 0.0, _ptr(t), _ptr(k), lt,
                                     None, None, _ptr(rank), None, None, m._stream()))
    return rank.cpu().numpy()


def raw_rank_scores(m, scores, tgt, tm, ex=(None, None)):
    import torch
    from poi_amd.models import _ptr
    n, lt = tgt.shape
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(m.device)
    s, t, k, eo, ei = dev(scores, torch.float32), dev(tgt, torch.int32), dev(tm, torch.int32), dev(ex[0], torch.int32), dev(ex[1], torch.int32)
    rank = torch.empty((n, lt), dtype=torch.int32, device=m.device)
    cnt = torch.empty(n, dtype=torch.int32, device=m.device)
    m.ctx.check(m.lib.poi_rank_scores(m.ctx.handle, _ptr(s), n, scores.shape[1], _ptr(t), _ptr(k), lt, _ptr(eo), _ptr(ei), _ptr(rank), _ptr(cnt), m._stream()))
    return rank.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("dim", [8, 64, 128])
def test_planted_ties_rank_by_index(pa, dim):
    n, N = 40, 300
    T, P, m, hts, sts, last = build(pa, 504 + dim, n, N, dim, False)
    rng = np.random.default_rng(dim)
    items = P["lt"][:N].astype(np.float32)
    tgt, tm = targets_of(504, T, 2)
    src = {}
    for r in range(n):                                    # copies of the targets' item rows, at ids below and above
        for j in rng.choice(N, 4, replace=False):
            if j not in tgt:
                items[j] = items[tgt[r, r % 2]]; src[int(j)] = int(tgt[r, r % 2])
    users = hts.astype(np.float32)
    sc32 = users.astype(np.float64) @ items.astype(np.float64).T
    for j, t in src.items():                              # (a BLAS may sum two equal columns in different orders)
        sc32[:, j] = sc32[:, t]
    # equal item rows give bitwise equal scores, so the exact ties of the float64 product are exact ties of the kernel; elsewhere the gap rule
    orc = RO.ranks(sc32, tgt, tm)
    got = raw_rank(m, users, items, tgt, tm, N, dim)
    tie_rows = [(r, i) for r in range(n) for i in range(2) if tm[r, i] and (sc32[r] == sc32[r, tgt[r, i]]).sum() > 1]
    assert len(tie_rows) >= n // 2
    clear = (orc["rank"] >= 0) & (orc["a"] == np.array([[(sc32[r] == sc32[r, tgt[r, i]]).sum() - 1 for i in range(2)] for r in range(n)]))
    assert clear[tuple(zip(*tie_rows))].mean() >= 0.9
    assert np.array_equal(got[clear], orc["rank"][clear])
    # ... and poi_rank_scores on explicit float32 rows with the same exact ties
    f32 = sc32.astype(np.float32)
    r2, c2 = raw_rank_scores(m, f32, tgt, tm)
    assert np.array_equal(r2, RO.ranks(f32.astype(np.float64), tgt, tm)["rank"]) and (c2 == N).all()


# ---- agreement with the existing paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [True, False])
def test_targets_from_the_own_topk_list_sit_at_their_position(pa, spatial):
    n, N = 70, 2049
    T, P, m, hts, sts, last = build(pa, 505, n, N, 64, spatial)
    sc = oracle_scores(P, T, hts, sts, last)
    ok = qualifying(sc)
    assert ok.mean() >= 0.9
    se = np.arange(n)
    idx = m.compute_sub_topk(se, K).cpu().numpy()
    pos = np.array([0, 7, K - 1])
    rank = m.compute_sub_target_rank(se, targets=idx[:, pos].copy()).cpu().numpy()
    assert np.array_equal(rank[ok], np.tile(pos, (ok.sum(), 1)))
    tes = T["test"][0]
    r = m.compute_sub_target_rank(se).cpu().numpy()[:, 0]
    for u in np.nonzero(ok)[0]:
        w = np.nonzero(idx[u] == tes[u, 0])[0]
        assert (len(w) and r[u] == w[0]) or (not len(w) and r[u] >= K)
    # poi_rank_scores on the device's own score matrix == a host count over that matrix, every row
    full = m.compute_sub_all_scores_device(se).cpu().numpy()
    tgt, tm = targets_of(505, T, 3)
    eo, ex = (t.cpu().numpy() for t in m.train_exclusion())
    for e in ((None, None), (eo, ex)):
        got, cnt = raw_rank_scores(m, full, tgt, tm, e)
        want = RO.ranks(full.astype(np.float64), tgt, tm, e[0], e[1])
        assert np.array_equal(got, want["rank"]) and np.array_equal(cnt, want["count"])


# ---- fallback models -------------------------------------------------------------------------------------------------------------------
def _own_list_check(m, se, rows_per_user=1):
    idx = m.compute_sub_topk(se, K).cpu().numpy()
    idx = idx.reshape(len(se), rows_per_user, K)
    lt = min(rows_per_user, m.tes_masks.shape[1])
    tgt = idx[:, :lt, 5].copy()
    rank, cnt = m.compute_sub_target_rank(se, targets=tgt.astype(np.int32), return_counts=True)
    assert np.array_equal(rank.cpu().numpy(), np.full((len(se), lt), 5)) and (cnt.cpu().numpy() == m.n_item).all()
    r = m.compute_sub_target_rank(se).cpu().numpy()
    tes, tm = m.tes_buys_masks.cpu().numpy()[se], m.tes_masks.cpu().numpy()[se]
    for u in range(len(se)):
        for i in range(min(lt, r.shape[1])):
            if tm[u, i]:
                w = np.nonzero(idx[u, i if rows_per_user > 1 else 0] == tes[u, i])[0]
                assert (len(w) and r[u, i] == w[0]) or (not len(w) and r[u, i] >= K), (u, i)
            else:
                assert r[u, i] == -1


def test_fallback_prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(45, 700, 14, 4)
    m = _model(ds)
    m.update_trained_items()
    _own_list_check(m, np.arange(3, 24, dtype=np.int32))


def test_fallback_carnn(pa):
    from tests.test_gpu_carnn import _model, _params
    T = toy_problem(540, n_user=21, n_item=150, n_dist=23, dim=32, len_max=9)
    rng = np.random.default_rng(9)
    coords = np.stack([40.0 + rng.random(150) * 0.05, -74.0 + rng.random(150) * 0.05], 1)
    m = _model(pa, T, _params(540, T), coords=coords)
    m.update_trained_items(); m.update_trained_dists()
    m.update_trained_users(m.predict(np.arange(21, dtype=np.int32)))
    _own_list_check(m, np.arange(21, dtype=np.int32))


def test_fallback_poi2vec(pa):
    from poi_amd import data as D, harness
    ds = D.make_poi2vec_synthetic(60, 200, 12, 13, local=0.9, n_nbr=8)
    m = harness.poi2vec_model(ds, dict(latent_size=20, seed=5, softmax_axis="items", eval_context="test"))
    m.update_trained_params()
    se = np.arange(5, 30, dtype=np.int32)
    _own_list_check(m, se, rows_per_user=m.compute_sub_topk(se, K).shape[0] // len(se))


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------------
def test_every_grid_gives_the_same_ranks(pa):
    n, N = 33, 2049
    T, P, m, hts, sts, last = build(pa, 506, n, N, 64, True)
    tgt, tm = targets_of(506, T, 3)
    eo, ex = m.train_exclusion()
    outs, splits = [], []
    try:
        for g in (0, 1, 3):
            m.ctx.set_option("rank_grid", g)
            outs.append(m.compute_sub_target_rank(np.arange(n), exclude="train", targets=(tgt, tm)).cpu().numpy())
            splits.append(m.ctx.last_plan("rank_splits"))
    finally:
        m.ctx.set_option("rank_grid", 0)
    assert splits[1] == 1 and splits[2] == 3 and splits[0] > 3, splits
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert (outs[0] >= 0).any()


# ---- contract edges ------------------------------------------------------------------------------------------------------------------------
def test_contract_edges(pa):
    import torch
    n, N = 5, 50
    T, P, m, hts, sts, last = build(pa, 507, n, N, 8, False)
    tgt = np.array([[3, 7], [N, 4], [-1, 9], [2, N], [1, 1]], np.int32)
    tm = np.array([[1, 0], [1, 1], [1, 1], [1, 0], [1, 1]], np.int32)
    rank = m.compute_sub_target_rank(np.arange(n), targets=(tgt, tm), sync=False).cpu().numpy()
    assert m.ctx.take_bad_ids(m._stream().value) == 2            # N and -1 under a set mask; the masked N is not read as an id
    assert rank[0, 1] == -1 and rank[1, 0] == -1 and rank[2, 0] == -1 and rank[3, 1] == -1
    assert (rank[[0, 1, 2, 3, 4, 4], [0, 1, 1, 0, 0, 1]] >= 0).all() and rank[4, 0] == rank[4, 1]
    with pytest.raises(IndexError):
        m.compute_sub_target_rank(np.arange(n), targets=(tgt, tm))
    with pytest.raises(pa._lib.PoiError):
        m.compute_sub_target_rank(np.arange(n), targets=np.zeros((n, 9), np.int32))
    from poi_amd.models import _ptr
    z = torch.zeros((1, 9), dtype=torch.int32, device=m.device)
    u = torch.zeros((1, 8), dtype=torch.float32, device=m.device)
    rc = m.lib.poi_score_rank(m.ctx.handle, _ptr(u), _ptr(m.trained_items.t), 1, N, m.kdim, None, None, None, None, None, None, 0, 0.0, _ptr(z), _ptr(z), 9,
                              None, None, _ptr(z), None, None, m._stream())
    assert rc == pa._lib.POI_ENOTSUP if hasattr(pa._lib, "POI_ENOTSUP") else rc != 0
    rc = m.lib.poi_score_rank(m.ctx.handle, _ptr(u), _ptr(m.trained_items.t), 0, N, m.kdim, None, None, None, None, None, None, 0, 0.0, _ptr(z), _ptr(z), 1,
                              None, None, _ptr(z), None, None, m._stream())
    assert rc == 0 and int(z.abs().sum()) == 0                   # n = 0: nothing runs, nothing is written


# ---- session ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [True, False])
def test_session_rank_of_equals_the_evaluation_rank(pa, spatial):
    import torch
    T = geo_problem(21, n_user=70, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    P = spatial_init(21, T) if spatial else gru_init(21, T)
    m = spatial_model(pa, T, P) if spatial else plain_model(pa, T, P)
    users = np.arange(T["n_user"])
    if spatial:
        hts, sts = m.predict_device(users)
        m.update_trained_users(hts); m.update_trained_sus(sts)
    else:
        m.update_trained_users(m.predict_device(users))
    s = m.session()
    s.load_history()
    tes = T["test"][0]
    for ids in (users, users[5:41], np.array([9, 3, 60, 17])):
        assert torch.equal(s.rank_of(ids, tes[ids]), m.compute_sub_target_rank(ids)), "rank_of != compute_sub_target_rank"


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [True, False])
def test_full_rank_metrics(pa, spatial):
    from poi_amd.evaluate import device_rank_metrics, full_rank_metrics
    n, N = 70, 300
    T, P, m, hts, sts, last = build(pa, 508, n, N, 64, spatial)
    sc = oracle_scores(P, T, hts, sts, last)
    tes = T["test"][0]
    orc = RO.ranks(sc, tes, np.ones_like(tes))
    ses = [np.arange(0, 32), np.arange(32, 70)]
    got = full_rank_metrics(m, ses, [5, 10, 20, 100, N])
    assert got["n"] == n and got["at"][N]["recall"] == 1.0
    dev = device_rank_metrics(m, ses, [5, 10, 20])
    assert qualifying(sc).all() and (orc["a"] == 0).all(), "the data of this test must be gap-qualified: pick another seed"
    for k in (5, 10, 20):
        assert got["at"][k]["hits"] == dev[k]["hits"] and abs(got["at"][k]["recall"] - dev[k]["recall"]) < 1e-12
        assert abs(got["at"][k]["ndcg"] - dev[k]["ndcg"]) < 1e-12
    ref = RO.summary(orc["rank"], orc["count"])
    for key in ("mrr", "auc_full", "mean_rank"):
        assert abs(got[key] - ref[key]) < 1e-12, key
    r = np.sort(orc["rank"].ravel())
    assert got["median_rank"] == r[(len(r) - 1) // 2]
