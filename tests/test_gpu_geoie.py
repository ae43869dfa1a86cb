"""GeoIE on the device (csrc/geoie.hip, models.OboGeoIE, harness.train_geoie) against the float64 oracle of tests/geoie_oracle.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from poi_amd import _lib, data as D, harness
from poi_amd.models import OboGeoIE
from tests import geoie_oracle as O
from tests.gpu_util import RTOL, assert_close, assert_step_close, delta_excess

pytestmark = pytest.mark.gpu

P_ = lambda t: ctypes.c_void_p(t.data_ptr())
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    return _lib.context(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Launch:
    """Device copies of a problem: tables, a / b, CSR, coordinates."""

    def __init__(self, P, seqs, coords):
        self.T = {k: torch.as_tensor(P[k], dtype=torch.float32).cuda().contiguous() for k in O.TABLES}
        self.ab = torch.tensor([P["a"], P["b"]], dtype=torch.float64, device="cuda")
        lens = np.array([len(s[0]) for s in seqs], np.int64)
        off = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        cat = lambda i: np.concatenate([np.asarray(s[i], np.int64) for s in seqs]) if off[-1] else np.zeros(0, np.int64)
        cv = lambda v: torch.as_tensor(np.asarray(v, np.int64).astype(np.int32)).cuda()
        self.lens, self.off, self.p, self.q = lens, cv(off), cv(np.append(cat(0), 0)), cv(np.append(cat(1), 0))
        self.coords = torch.as_tensor(np.ascontiguousarray(coords, np.float64)).cuda()
        self.cphi = torch.as_tensor(D.cos_lat(coords)).cuda()
        self.n_user, self.n_item, self.dim = len(seqs), P["g"].shape[0] - 1, P["g"].shape[1]

    def prm(self):
        return _lib.GeoieParams(*[P_(self.T[k]) for k in O.TABLES], P_(self.ab), self.n_user, self.n_item, self.dim)

    def step(self, ctx, users, alpha=0.01, lam=0.001, d_min=0.0, rows=None):
        users = np.asarray(users, np.int64)
        uu = torch.as_tensor(users.astype(np.int32)).cuda()
        if rows is None:
            rows = int(np.maximum(self.lens[np.clip(users, 0, self.n_user - 1)] - 1, 0)[(users >= 0) & (users < self.n_user)].sum())
        loss = torch.empty(len(users), dtype=torch.float32, device="cuda")
        prm = self.prm()
        ctx.check(ctx.lib.poi_geoie_step(ctx.handle, ctypes.byref(prm), P_(self.off), P_(self.p), P_(self.q), P_(self.coords), P_(self.cphi),
                                         P_(uu), len(users), rows, alpha, lam, d_min, P_(loss), _stream()))
        return loss.cpu().numpy()

    def host(self):
        out = {k: self.T[k].cpu().numpy().astype(np.float64) for k in O.TABLES}
        a, b = self.ab.cpu().numpy()
        out["a"], out["b"] = float(a), float(b)
        return out


def _problem(seed, n_user, n_item, dim, lens, revisit=0.3, b=None):
    rng = np.random.default_rng(seed)
    P = O.round_f32(O.init_tables(rng, n_user, n_item, dim))
    if b is not None:
        P["b"] = float(b)
    coords = np.stack([40 + 0.3 * rng.random(n_item), -74 + 0.4 * rng.random(n_item)], 1)
    seqs = []
    for L in lens:
        p = rng.integers(0, n_item, L) if revisit > 0 else rng.permutation(n_item)[:L]
        rep = rng.random(L) < revisit
        for i in np.nonzero(rep)[0]:
            if i > 0:
                p[i] = p[rng.integers(0, i)]                                               # revisits: zero-distance pairs
        own = set(p.tolist())
        q = rng.integers(0, n_item, L)
        for i in range(L):
            while q[i] in own:
                q[i] = rng.integers(0, n_item)
        seqs.append((p, q))
    return P, seqs, coords


def _check_step(got, Q, P, what, absmass=None):
    assert_step_close(got, Q, P, ("g", "h", "z"), what, absmass=absmass)
    for k in ("a", "b"):
        assert abs(got[k] - Q[k]) <= 1e-6 * max(abs(Q[k]), 1e-3) + 1e-5 * abs(Q[k] - P[k]), (k, what, got[k], Q[k], P[k])
    np.testing.assert_array_equal(got["t"], P["t"])


@pytest.mark.parametrize("dim", [4, 20, 64, 128])
@pytest.mark.parametrize("L", [2, 3, 17, 1300])
def test_one_user_launch_equals_the_reference_step(ctx, dim, L):
    ctx.set_batch_cap(1)
    n_item = 3000 if L == 1300 else 200
    P, seqs, coords = _problem(dim * 7 + L, 4, n_item, dim, [5, L, 3, 9], b=0.3)            # b > 0 with revisits (zero distances)
    X = Launch(P, seqs, coords)
    loss = X.step(ctx, [1])
    Q, ref = O.step(P, *seqs[1], coords, 0.01, 0.001)
    assert np.isfinite(ref)
    assert_close(loss, [ref], "loss %d/%d" % (dim, L), rtol=RTOL if L < 1300 else 1e-4)
    _check_step(X.host(), Q, P, "D=%d L=%d" % (dim, L))


@pytest.mark.parametrize("dim", [20, 64])
def test_negative_b_with_d_min(ctx, dim):
    ctx.set_batch_cap(1)
    P, seqs, coords = _problem(dim, 3, 150, dim, [4, 40, 6], b=-0.35)
    X = Launch(P, seqs, coords)
    loss = X.step(ctx, [1], d_min=0.01)
    Q, ref = O.step(P, *seqs[1], coords, 0.01, 0.001, d_min=0.01)
    assert np.isfinite(ref)
    assert_close(loss, [ref], "loss")
    _check_step(X.host(), Q, P, "b<0, d_min")


@pytest.mark.parametrize("cap", [1.0, 64.0, 1e9])
def test_batched_launch_follows_the_capped_rule(ctx, cap):
    rng = np.random.default_rng(int(min(cap, 77)))
    lens = np.concatenate([[0, 1, 1, 2, 1300, 700], rng.integers(2, 60, 120)])
    P, seqs, coords = _problem(11, len(lens), 400, 20, lens, b=0.2)
    X = Launch(P, seqs, coords)
    users = rng.permutation(len(lens))
    ctx.set_batch_cap(cap)
    try:
        ctx.take_bad_ids()
        loss = X.step(ctx, users)
        assert ctx.take_bad_ids() == 0
    finally:
        ctx.set_batch_cap(1)
    Q, ref, M = O.batch_step(P, [seqs[u] for u in users], coords, 0.01, 0.001, cap=cap, absmass=True)
    short = np.array([len(seqs[u][0]) < 2 for u in users])
    assert np.all(loss[short] == 0)
    np.testing.assert_allclose(loss, ref, rtol=1e-4, atol=1e-5)
    got = X.host()
    _check_step(got, Q, P, "cap %g" % cap, absmass=M)
    # z moves by decay only: its update is a multiple of the row
    moved = np.nonzero(np.any(got["z"] != P["z"], axis=1))[0]
    ratio = got["z"][moved] / P["z"][moved]
    assert np.allclose(ratio, ratio[:, :1], rtol=0, atol=2e-6)


def test_rejection_moves_nothing_and_removal_is_bitwise_equal(ctx):
    P, seqs, coords = _problem(3, 8, 120, 20, [6, 9, 30, 12, 5, 20, 8, 15], revisit=0.0, b=-0.1)
    # user 2 revisits p_0 (a zero distance at b <= 0); user 5 has an out-of-range POI
    seqs[2][0][7] = seqs[2][0][0]
    bad_p = seqs[5][0].copy(); bad_p[3] = 120
    seqs[5] = (bad_p, seqs[5][1])
    ctx.set_batch_cap(64)
    try:
        for rejected in (2, 5):
            users = np.array([0, 1, rejected, 3, 4, 6, 7])
            X = Launch(P, seqs, coords)
            ctx.take_bad_ids()
            loss = X.step(ctx, users)
            k = int(np.nonzero(users == rejected)[0][0])
            assert np.isnan(loss[k]) and np.all(np.isfinite(np.delete(loss, k)))
            assert ctx.take_bad_ids() == 1
            Y = Launch(P, seqs, coords)
            loss2 = Y.step(ctx, np.delete(users, k))
            assert np.array_equal(np.delete(loss, k), loss2)
            for t in O.TABLES:
                assert torch.equal(X.T[t], Y.T[t]), (rejected, t)
            assert torch.equal(X.ab, Y.ab)
            # alone it moves nothing at all
            Z = Launch(P, seqs, coords)
            Z.step(ctx, [rejected])
            assert ctx.take_bad_ids() == 1
            for t in O.TABLES:
                assert torch.equal(Z.T[t], torch.as_tensor(P[t], dtype=torch.float32).cuda()), t
            assert Z.ab.cpu().tolist() == [P["a"], P["b"]]
        # a user id out of the table
        X = Launch(P, seqs, coords)
        loss = X.step(ctx, [0, 8], rows=5)
        assert np.isnan(loss[1]) and np.isfinite(loss[0]) and ctx.take_bad_ids() == 1
    finally:
        ctx.set_batch_cap(1)


def test_identical_launches_are_bitwise_identical(ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(2, 200, 300)
    P, seqs, coords = _problem(9, len(lens), 60, 64, lens, b=0.15)                           # 60 POIs: long runs of equal keys
    ctx.set_batch_cap(64)
    try:
        X, Y = Launch(P, seqs, coords), Launch(P, seqs, coords)
        l1, l2 = X.step(ctx, np.arange(len(lens))), Y.step(ctx, np.arange(len(lens)))
    finally:
        ctx.set_batch_cap(1)
    assert np.array_equal(l1, l2)
    for t in O.TABLES:
        assert torch.equal(X.T[t], Y.T[t]), t
    assert torch.equal(X.ab, Y.ab)


@pytest.mark.parametrize("case,split", [("s1", -1), ("s2", -2)])
def test_device_pair_distances_within_one_ulp_of_golden(ctx, case, split):
    g = np.load(os.path.join(GOLDEN, "geoie_pairs.npz"))
    G = lambda k: g[case + "_" + k]
    ds, alias = D.load_sequence_file(os.path.join(GOLDEN, "sequences_small.txt"), split=split, seed=1, return_aliases=True)
    ours = np.array([alias[str(r)] for r in G("ref_ids")] + [ds.n_item])
    msk = G("tra_masks").astype(bool)
    q = ours[G("tra_neg")][msk]
    n = ds.n_user
    off = torch.as_tensor(np.asarray(ds.off, np.int32)).cuda()
    pp, qq = (torch.as_tensor(np.asarray(v, np.int32)).cuda() for v in (ds.tra_p, q))
    xy = torch.as_tensor(ds.coords).cuda()
    cphi = torch.as_tensor(D.cos_lat(ds.coords)).cuda()
    order = np.arange(n)[::-1].copy()                                                      # any user order: packed per launch order
    rows = np.maximum(ds.lens[order] - 1, 0)
    npair = int((rows * (rows + 1) // 2).sum())
    dp, dq = (torch.empty(npair, dtype=torch.float32, device="cuda") for _ in range(2))
    users = torch.as_tensor(order.astype(np.int32)).cuda()
    ctx.check(ctx.lib.poi_geoie_pair_distances(ctx.handle, P_(off), P_(pp), P_(qq), n, ds.n_item, P_(xy), P_(cphi), P_(users), n, int(rows.sum()),
                                               npair, P_(dp), P_(dq), _stream()))
    hdp, hdq, _, _ = D.geoie_pair_distances(ds.coords, ds.off, ds.tra_p, q, order)
    # the golden in launch order
    gpo = np.zeros(n + 1, np.int64)
    r_all = np.maximum(ds.lens - 1, 0)
    np.cumsum(r_all * (r_all + 1) // 2, out=gpo[1:])
    want_p = np.concatenate([G("dp")[gpo[u]:gpo[u + 1]] for u in order]).astype(np.float32)
    want_q = np.concatenate([G("dq")[gpo[u]:gpo[u + 1]] for u in order]).astype(np.float32)
    for got, want, host in ((dp.cpu().numpy(), want_p, hdp), (dq.cpu().numpy(), want_q, hdq)):
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        assert np.abs(got.view(np.int32).astype(np.int64) - host.view(np.int32).astype(np.int64)).max() <= 1


def _model(ds, dim=20, seed=3, **kw):
    return OboGeoIE(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_in=dim, n_hidden=dim,
                    coords=ds.coords, seed=seed, **kw)


@pytest.mark.parametrize("norm", ["reference", "count"])
def test_user_vectors_and_scores(ctx, norm):
    ds = D.make_synthetic(70, 900, 30, 5)
    m = _model(ds, dim=20, score_norm=norm)
    m.train_batch(np.arange(ds.n_user))
    m.update_trained()
    Pt = {k: m._trained[k].cpu().numpy().astype(np.float64) for k in O.TABLES}
    uv = m.user_vectors().cpu().numpy()
    want = O.user_vectors(Pt, ds.off, ds.tra_p, m.len_max, norm)
    assert_close(uv, want, "user vectors " + norm)
    se = np.arange(5, 60, dtype=np.int32)
    sc = m.compute_sub_all_scores(se)
    ref = O.scores(Pt, want[se])
    assert_close(sc, ref, "scores " + norm)
    idx, tsc = m.compute_sub_topk(se, 20, return_scores=True)
    assert np.array_equal(tsc.cpu().numpy(), np.take_along_axis(sc, idx.cpu().numpy().astype(np.int64), 1))
    assert np.all(np.diff(tsc.cpu().numpy(), axis=1) <= 0)
    assert not m.compute_sub_auc_preference(se).any()
    Pl = dict(Pt, **{k: getattr(m, k).t.cpu().numpy().astype(np.float64) for k in O.TABLES})
    Pl["a"], Pl["b"] = float(m.a.get_value()), float(m.b.get_value())
    assert np.isclose(m.l2.eval(), O.l2(Pl, 0.001), rtol=1e-6)


def test_train_geoie_learns(ctx):
    ds = D.make_synthetic(600, 800, 40, 13, local=0.9, n_nbr=8)
    logs = []
    p = dict(epochs=4, batch=128, latent_size=20, alpha=0.05, seed=5, score_norm="count", d_min=0.01, batch_size_test=64)
    model, best, hist = harness.train_geoie(ds, p, log=logs.append)
    losses = [h["loss"] for h in hist]
    assert all(np.isfinite(losses)) and losses[-1] > losses[0], losses
    assert all(h["auc"] == 0.0 for h in hist) and all(h["rejected"] == 0 for h in hist)
    assert all(np.isfinite([h["a"], h["b"]]).all() for h in hist)
    r20 = [h["recall"][20] for h in hist]
    # an untrained model (uniform(-0.5, 0.5) tables) ranks by noise.  Measured on MI355X: untrained recall@20 0.028; after the epochs
    # 0.030, 0.035, 0.048, 0.053.  (t never moves and z only decays - GeoIE.py's cost - so the t.z half of the score stays noise and
    # only m_u.h learns.)  The bar: 1.5x the untrained model, and rising.
    untrained = _model(ds, dim=20, seed=5, score_norm="count")
    untrained.update_trained()
    from poi_amd.evaluate import device_rank_metrics
    ses = harness.compute_start_end(ds.n_user, 64)
    r0 = device_rank_metrics(untrained, ses, [20])[20]["recall"]
    assert r20[-1] > 1.5 * r0 and r20[-1] > r20[0], (r20, r0)
    assert len(logs) == 4 and "sum_loss" in logs[0] and "rejected users 0" in logs[0]


def test_one_user_epoch_matches_sequential_oracle_steps(ctx):
    ds = D.make_synthetic(6, 80, 12, 21)
    ctx.set_batch_cap(1)
    m = _model(ds, dim=8, seed=2, d_min=0.01)
    P = {k: getattr(m, k).t.cpu().numpy().astype(np.float64) for k in O.TABLES}
    P["a"], P["b"] = float(m.a.get_value()), float(m.b.get_value())
    off = np.asarray(ds.off, np.int64)
    Q = P
    for u in np.random.default_rng(1).permutation(ds.n_user):
        loss = m.train(int(u))
        Q, ref = O.step(Q, ds.tra_p[off[u]:off[u + 1]], ds.tra_q[off[u]:off[u + 1]], ds.coords, 0.01, 0.001, d_min=0.01)
        assert abs(loss - ref) <= 1e-4 * max(1.0, abs(ref)), (u, loss, ref)
    got = {k: getattr(m, k).t.cpu().numpy().astype(np.float64) for k in O.TABLES}
    for k in ("g", "h", "z"):
        assert_close(got[k], Q[k], k)
    np.testing.assert_array_equal(got["t"], P["t"])
    assert abs(float(m.a.get_value()) - Q["a"]) <= 1e-6 and abs(float(m.b.get_value()) - Q["b"]) <= 1e-6
