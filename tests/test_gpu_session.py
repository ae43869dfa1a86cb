"""-m gpu tests of the online sessions (models.Session -> poi_session_advance / poi_session_sts): per-slot GRU state advanced one
check-in at a time must equal the float64 oracle's `predict` on the same sequence, run from the float32-rounded tables
(tests/gpu_util.round_f32) - state within RTOL, last_poi / steps / top-K lists exact.  Nothing here compares the code under test
with itself, except where the statement IS an identity of two of its paths (recommend after load_history == compute_sub_topk)."""
import numpy as np
import pytest

from oracle import poi_oracle as O
from tests.gpu_util import RTOL, assert_close, round_f32

pytestmark = pytest.mark.gpu

K = 20


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


# ---- problems ----------------------------------------------------------------------------------------------------------------------
def geo_problem(seed, n_user, n_item, n_dist, dim, len_min, len_max, box_km=40.0):
    """Padded tables in the reference layout with POI coordinates in a box and the train bins of data.dist_pos_bins.  The bin width is
    30 km / n_dist, so in a 40 km box the bins are neither all 0 nor all clipped to n_dist."""
    from poi_amd import data
    rng = np.random.default_rng(seed)
    lens = rng.integers(len_min, len_max + 1, n_user)
    lens[0] = len_max
    coords = np.stack((30.0 + rng.uniform(0, box_km / 111.0, n_item), 120.0 + rng.uniform(0, box_km / 96.0, n_item)), axis=1)
    dd_m = 30000.0 / n_dist
    P = np.full((n_user, len_max), n_item); Q = P.copy(); M = np.zeros((n_user, len_max), int)
    for u, L in enumerate(lens):
        P[u, :L] = rng.integers(0, n_item, L); Q[u, :L] = rng.integers(0, n_item, L); M[u, :L] = 1
    off, p_flat = data.padded_to_csr(P, lens)
    _, q_flat = data.padded_to_csr(Q, lens)
    dp = data.dist_pos_bins(off, p_flat, coords, dd_m, n_dist)
    dq = data.dist_neg_bins(off, p_flat, q_flat, coords, dd_m, n_dist)
    DP = np.full((n_user, len_max), n_dist); DQ = DP.copy()
    for u, L in enumerate(lens):
        DP[u, :L] = dp[off[u]:off[u] + L]; DQ[u, :L] = dq[off[u]:off[u] + L]
    inner = np.concatenate([DP[u, 1:L] for u, L in enumerate(lens)])
    assert 0 < (inner == n_dist).mean() < 1 and len(np.unique(inner)) > 3, "bins must be neither all 0 nor all clipped"
    tes_p = rng.integers(0, n_item, (n_user, 1)); tes_q = rng.integers(0, n_item, (n_user, 1))
    last = P[np.arange(n_user), lens - 1]
    tes_d = data.cal_dis_vec(coords[tes_p[:, 0], 0], coords[tes_p[:, 0], 1], coords[last, 0], coords[last, 1], dd_m, n_dist)[:, None]
    return dict(train=[P, M, Q], test=[tes_p, np.ones((n_user, 1), int), tes_q], dist=[DP, tes_d, DQ], lens=lens, off=np.asarray(off), p_flat=np.asarray(p_flat),
                coords=coords, dd_m=dd_m, n_user=n_user, n_item=n_item, n_dist=n_dist, dim=dim, len_max=len_max)


def spatial_init(seed, T, bias=True):
    rng = np.random.default_rng(seed + 1000)
    P = O.init_spatial_params(rng, T["n_item"], T["n_dist"], T["dim"])      # the reference's uniform(-0.5, 0.5)
    if bias:
        P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape); P["bs"] = rng.uniform(-0.2, 0.2, P["bs"].shape)
    return round_f32(P)


def gru_init(seed, T):
    rng = np.random.default_rng(seed + 2000)
    P = O.init_gru_params(rng, T["n_item"], T["dim"])
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape)
    return round_f32(P)


def spatial_model(pa, T, P, **kw):
    m = pa.models.OboSpatialGru(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                                n_dists=[T["n_dist"], T["dd_m"] / 1000.0], n_in=T["dim"], n_hidden=T["dim"], init=P, coords=T["coords"], **kw)
    m.update_trained_items(); m.update_trained_dists()
    return m


def plain_model(pa, T, P, cls="OboGru", **kw):
    m = getattr(pa.models, cls)(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                                n_in=T["dim"], n_hidden=T["dim"], init=P, **kw)
    m.update_trained_items()
    return m


def seq_bins(T, seq):
    """dp of a sequence: n_dist at position 0, then bin(coords[p_t], coords[p_{t-1}])."""
    from poi_amd import data
    seq = np.asarray(seq)
    c = T["coords"]
    out = np.full(len(seq), T["n_dist"], np.int64)
    if len(seq) > 1:
        out[1:] = data.cal_dis_vec(c[seq[1:], 0], c[seq[1:], 1], c[seq[:-1], 0], c[seq[:-1], 1], T["dd_m"], T["n_dist"])
    return out


def oracle_rows(P, T, seqs, spatial=True):
    """The oracle's predict on explicit sequences -> (hts, sts | None)."""
    hs, ss = [], []
    for s in seqs:
        s = list(s)
        if spatial:
            h, st = O.spatial_predict(P, P["lt"], P["di"], [s], [seq_bins(T, s)], [np.ones(len(s), int)])
            hs.append(h[0]); ss.append(st[0])
        else:
            hs.append(O.gru_predict(P, P["lt"], [s], [np.ones(len(s), int)])[0])
    return np.array(hs), (np.array(ss) if spatial else None)


def oracle_scores(P, T, hts, sts, last):
    """float64 scores of every POI: h . items[:-1]^T (+ wd * sts[bin(last, .)] for bins below n_dist)."""
    from poi_amd import data
    sc = O.score_all(hts, P["lt"])
    if sts is not None:
        c = T["coords"]
        ul = np.stack([data.cal_dis_vec(c[l, 0], c[l, 1], c[:, 0], c[:, 1], T["dd_m"], T["n_dist"]) for l in last])
        sc = sc + P["wd"] * O.acquire_prob(sts, ul, T["n_dist"])
    return sc


def qualifying(sc, k=K):
    """Rows whose top-(k+1) adjacent gaps are >= 1e-6 max|score| (the rule of test_gpu_fullsize.py): a float32 kernel must rank them exactly."""
    top = -np.sort(-sc, axis=1)[:, :k + 1]
    return (top[:, :-1] - top[:, 1:]).min(axis=1) >= 1e-6 * np.abs(sc).max()


def seqs_of(T):
    return [T["train"][0][u, :L] for u, L in enumerate(T["lens"])]


# ---- 1 - 3: replay == predict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dist,dim", [(11, 8), (11, 20), (200, 20), (200, 128), (11, 128)])
def test_replay_equals_predict_spatial(pa, n_dist, dim):
    T = geo_problem(3 + dim + n_dist, n_user=24, n_item=50, n_dist=n_dist, dim=dim, len_min=4, len_max=12)
    P = spatial_init(dim, T)
    m = spatial_model(pa, T, P)
    s = m.session()
    s.replay(T["off"], T["p_flat"])
    hts, sts = oracle_rows(P, T, seqs_of(T))
    st = s.state()
    print("replay spatial dim %d bins %d: h %.2e sts %.2e" % (dim, n_dist, np.abs(st["h"] - hts).max() / np.abs(hts).max(), np.abs(st["sts"] - sts).max() / sts.max()))
    assert_close(st["h"], hts, "h"); assert_close(st["sts"], sts, "sts")
    assert np.array_equal(st["last_poi"], [q[-1] for q in seqs_of(T)]) and np.array_equal(st["steps"], T["lens"])
    if m.kdim != dim:          # stored padded: the pad columns of the state stay exactly zero
        assert m.kdim == 64 and s.h.shape[1] == 64 and float(s.h[:, dim:].abs().max()) == 0.0


@pytest.mark.parametrize("cls,dim", [("OboGru", 8), ("OboGru", 64), ("Gru", 8), ("Gru", 64)])
def test_replay_equals_predict_plain(pa, cls, dim):
    T = geo_problem(40 + dim, n_user=24, n_item=50, n_dist=11, dim=dim, len_min=4, len_max=12)
    P = gru_init(dim, T)
    m = plain_model(pa, T, P, cls)
    s = m.session()
    s.replay(T["off"], T["p_flat"])
    hts, _ = oracle_rows(P, T, seqs_of(T), spatial=False)
    st = s.state()
    assert_close(st["h"], hts, "h")
    assert np.array_equal(st["last_poi"], [q[-1] for q in seqs_of(T)]) and np.array_equal(st["steps"], T["lens"]) and "sts" not in st


def test_long_saturated_sequences(pa):
    """D = 128, lengths up to 50, the reference's uniform(-0.5, 0.5) init: the regime where a float32 recurrence lands 1e-5 .. 1e-4 off
    (tests/gpu_util.py).  Same RTOL."""
    T = geo_problem(77, n_user=40, n_item=300, n_dist=200, dim=128, len_min=20, len_max=50)
    P = spatial_init(77, T, bias=False)
    m = spatial_model(pa, T, P)
    s = m.session()
    s.replay(T["off"], T["p_flat"])
    hts, sts = oracle_rows(P, T, seqs_of(T))
    st = s.state()
    print("saturated: h %.2e sts %.2e" % (np.abs(st["h"] - hts).max() / np.abs(hts).max(), np.abs(st["sts"] - sts).max() / sts.max()))
    assert_close(st["h"], hts, "h"); assert_close(st["sts"], sts, "sts")


# ---- 4: both launch regimes and the switch ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def regimes(pa):
    """600 slots with a history of 1 .. 3 check-ins and one further event for each: the oracle's state before and after."""
    T = geo_problem(5, n_user=600, n_item=80, n_dist=11, dim=32, len_min=1, len_max=3)
    P = spatial_init(5, T)
    rng = np.random.default_rng(50)
    ev = rng.integers(0, T["n_item"], T["n_user"])
    h1, s1 = oracle_rows(P, T, [list(q) + [e] for q, e in zip(seqs_of(T), ev)])
    return T, P, ev, h1, s1


def _snapshot(s):
    return [t.clone() for t in (s.h, s.sts, s.last_poi, s.steps)]


@pytest.mark.parametrize("n,tile_min", [(1, None), (511, None), (512, None), (513, None), (77, 16), (513, 1 << 30), (600, 1 << 30)])
def test_both_launch_regimes_and_the_switch(pa, regimes, n, tile_min):
    """n just below / at / above the switch point read from the plan, n = 1, n not a multiple of the 16-event tile; and both kernels
    forced onto sizes of the other side (option "session_tile_min").  Named slots match the oracle, the others keep every bit."""
    import torch
    T, P, ev, h1, s1 = regimes
    m = spatial_model(pa, T, P)
    s = m.session()
    s.replay(T["off"], T["p_flat"])                 # 600 / 400 / 200 events per step
    default = m.ctx.last_plan("session_tile_min")
    assert m.ctx.last_plan("session_path") == (1 if int((T["lens"] == 3).sum()) >= default else 0)      # the replay's last launch
    if tile_min is None:
        assert default == 512, "the cases of this test stand around the default switch point"
    else:
        m.ctx.set_option("session_tile_min", tile_min)
    try:
        named = np.random.default_rng(n).permutation(T["n_user"])[:n]
        before = _snapshot(s)
        s.advance(named, ev[named])
        switch = m.ctx.last_plan("session_tile_min")
        assert switch == (default if tile_min is None else tile_min)
        assert m.ctx.last_plan("session_path") == (1 if n >= switch else 0)
        assert m.ctx.last_plan("session_tiles") == ((n + 15) // 16 if n >= switch else 0)
    finally:
        m.ctx.set_option("session_tile_min", default)
    st = s.state(named)
    assert_close(st["h"], h1[named], "h"); assert_close(st["sts"], s1[named], "sts")
    assert np.array_equal(st["last_poi"], ev[named]) and np.array_equal(st["steps"], T["lens"][named] + 1)
    rest = torch.as_tensor(np.setdiff1d(np.arange(T["n_user"]), named)).to(s.h.device)
    for a, b in zip(before, _snapshot(s)):
        assert torch.equal(a[rest], b[rest]), "a slot the call did not name changed"


# ---- 5: incremental == batch --------------------------------------------------------------------------------------------------------
def test_incremental_equals_batch(pa):
    T = geo_problem(9, n_user=30, n_item=50, n_dist=11, dim=20, len_min=4, len_max=10)
    P = spatial_init(9, T)
    m = spatial_model(pa, T, P)
    s = m.session()
    s.load_history()
    st = s.state()
    assert np.array_equal(st["last_poi"], [q[-1] for q in seqs_of(T)]) and np.array_equal(st["steps"], T["lens"])
    rng = np.random.default_rng(90)
    new = rng.integers(0, T["n_item"], T["n_user"])
    hts, sts = s.advance(np.arange(T["n_user"]), new, return_state=True)
    eh, es = oracle_rows(P, T, [list(q) + [e] for q, e in zip(seqs_of(T), new)])
    st = s.state()
    assert_close(st["h"], eh, "h"); assert_close(st["sts"], es, "sts")
    assert_close(hts[:, :T["dim"]].cpu().numpy(), eh, "hts_out"); assert_close(sts.cpu().numpy(), es, "sts_out")
    # the same user twice in one call, different POIs: applied in the order of the call (and user 5 once, in between)
    a, b, c = 7, 41, 13
    s.advance([3, 5, 3], [a, c, b])
    e2, s2 = oracle_rows(P, T, [list(seqs_of(T)[3]) + [new[3], a, b], list(seqs_of(T)[5]) + [new[5], c]])
    st = s.state([3, 5])
    assert_close(st["h"], e2, "h after a repeated slot"); assert_close(st["sts"], s2, "sts after a repeated slot")
    assert np.array_equal(st["last_poi"], [b, c]) and np.array_equal(st["steps"], T["lens"][[3, 5]] + [3, 2])


def test_seed_recomputes_the_head(pa):
    T = geo_problem(12, n_user=8, n_item=50, n_dist=11, dim=8, len_min=4, len_max=6)
    P = spatial_init(12, T)
    m = spatial_model(pa, T, P)
    hts, sts = oracle_rows(P, T, seqs_of(T))
    s = m.session(n_slot=20)
    s.seed(np.arange(8) + 10, hts, [q[-1] for q in seqs_of(T)], T["lens"])
    st = s.state(np.arange(8) + 10)
    assert_close(st["sts"], np.array([O.softmax0(P["vs"] @ np.float64(h) + P["bs"]) for h in st["h"]]), "sts")
    assert np.array_equal(st["steps"], T["lens"]) and float(s.h[:10].abs().max()) == 0.0


# ---- 6: recommend -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [True, False])
@pytest.mark.parametrize("dim", [32, 128])
def test_recommend_matches_the_oracle_ranks(pa, spatial, dim):
    T = geo_problem(60 + dim, n_user=64, n_item=300, n_dist=11, dim=dim, len_min=4, len_max=8)
    P = spatial_init(dim, T) if spatial else gru_init(dim, T)
    m = spatial_model(pa, T, P) if spatial else plain_model(pa, T, P)
    hts, sts = oracle_rows(P, T, seqs_of(T), spatial=spatial)
    sc = oracle_scores(P, T, hts, sts, [q[-1] for q in seqs_of(T)])
    ok = qualifying(sc)
    assert ok.mean() >= 0.95, "only %.1f %% of the oracle's rows have clear top-%d gaps: pick another seed" % (100 * ok.mean(), K)
    s = m.session(n_slot=T["n_user"] + 3)
    s.replay(T["off"], T["p_flat"])
    idx = s.recommend(np.arange(T["n_user"]), K).cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == (T["n_user"], K)
    assert np.array_equal(idx[ok], O.topk_desc(sc, K)[ok])
    # no check-in yet: 0 . items and no distance term - all ties, ascending index
    assert np.array_equal(s.recommend([T["n_user"], T["n_user"] + 2], K).cpu().numpy(), np.tile(np.arange(K), (2, 1)))
    # k > 32 goes through explicit score rows
    top40 = s.recommend(np.arange(T["n_user"]), 40).cpu().numpy()
    ok40 = qualifying(sc, 40)
    assert ok40.any() and np.array_equal(top40[ok40], O.topk_desc(sc, 40)[ok40])


@pytest.mark.parametrize("spatial", [True, False])
def test_recommend_after_load_history_is_the_evaluation_ranking(pa, spatial):
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
    for ids in (users, users[5:41], np.array([9, 3, 60, 17])):
        assert torch.equal(s.recommend(ids, K), m.compute_sub_topk(ids, K)), "recommend != compute_sub_topk"


# ---- 7: contract edges --------------------------------------------------------------------------------------------------------------
def test_contract_edges(pa):
    import torch
    T = geo_problem(31, n_user=12, n_item=50, n_dist=11, dim=8, len_min=4, len_max=6)
    P = spatial_init(31, T)
    m = spatial_model(pa, T, P)
    s = m.session()
    s.replay(T["off"], T["p_flat"])
    before = _snapshot(s)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(s.h.device)
    for slots, pois in (([0, 12], [1, 2]), ([0, -1], [1, 2]), ([0, 1], [1, 50]), ([0, 1], [-1, 2]),                  # checked on the host
                        (dev([0, 12]), dev([1, 2])), (dev([0, 1]), dev([1, 50])), (dev([4, 2, 4]), dev([1, 2, 3]))):   # ... by the kernel
        with pytest.raises(IndexError):
            s.advance(slots, pois)
        rows = [4] if isinstance(slots, torch.Tensor) and slots.numel() == 3 else [1] if isinstance(slots, torch.Tensor) else range(12)
        for a, b in zip(before, _snapshot(s)):      # the offending slots keep every bit (host-checked calls move nothing at all)
            assert torch.equal(a[list(rows)], b[list(rows)])
        s.reset(); s.replay(T["off"], T["p_flat"])
        for a, b in zip(before, _snapshot(s)):      # and two identical replays give bit-identical state
            assert torch.equal(a, b)
    # NaN rows for the rejected events of a device batch
    hts, sts = s.advance(dev([0, 12]), dev([1, 2]), sync=False, return_state=True)
    assert m.ctx.take_bad_ids() == 1
    assert torch.isnan(hts[1]).all() and torch.isnan(sts[1]).all() and torch.isfinite(hts[0]).all()
    # out of scope / missing coordinates
    M = pa.models
    with pytest.raises(pa._lib.PoiError, match="coords"):
        M.OboSpatialGru(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                        n_dists=[T["n_dist"], 0.2], n_in=8, n_hidden=8).session()
    with pytest.raises(pa._lib.PoiError, match="out of scope"):
        M.Lstm(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"], n_in=8, n_hidden=8).session()
    with pytest.raises(pa._lib.PoiError, match="out of scope"):
        M.OboCARNN(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                   n_dists=[T["n_dist"], 0.2], n_in=8, n_hidden=8, coords=T["coords"]).session()


def test_session_follows_the_snapshots(pa):
    T = geo_problem(33, n_user=12, n_item=50, n_dist=11, dim=8, len_min=4, len_max=6)
    P = spatial_init(33, T)
    m = spatial_model(pa, T, P)
    s = m.session()
    for u in (0, 3, 5, 3):
        m.train(u)
    par = {k: np.float64(getattr(m, k).get_value()) for k in ("lt", "di", "ui", "wh", "bi", "vs", "bs")}
    assert np.abs(par["lt"] - P["lt"]).max() > 0
    s.replay(T["off"], T["p_flat"])                 # snapshots still hold the initial tables; ui / wh / bi / vs / bs are live
    hts, sts = oracle_rows({**P, **par, "lt": P["lt"], "di": P["di"]}, T, seqs_of(T))
    assert_close(s.state()["h"], hts, "h on the old snapshot")
    m.update_trained_items(); m.update_trained_dists()
    s.reset(); s.replay(T["off"], T["p_flat"])
    hts, sts = oracle_rows({**P, **par}, T, seqs_of(T))
    st = s.state()
    assert_close(st["h"], hts, "h on the new snapshot"); assert_close(st["sts"], sts, "sts on the new snapshot")
    for k in par:                                    # a session never changes a model parameter
        assert np.array_equal(np.float64(getattr(m, k).get_value()), par[k])
