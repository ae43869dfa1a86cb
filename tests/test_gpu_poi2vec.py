"""POI2Vec on the device (csrc/poi2vec.hip, models.OboPoi2vec, harness.train_poi2vec) against the float64 oracle of tests/poi2vec_oracle.py.

Discontinuities: ind_i = ceil(|mean c_i|), floor(1 - S_i) and (scoring) ceil(|z_n|) are decided on float64 values on the device.  Every
parity input is generated so that, in the oracle, those values stay at least 1e-9 away from an integer (asserted by _margins_ok; the
next seed is taken otherwise); values that are exactly 0 on both sides (an empty context, a product through it) are sums of nothing and
cannot flip.  No row is excluded anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from poi_amd import _lib, data as D, harness
from poi_amd.models import OboPoi2vec
from tests import poi2vec_oracle as O
from tests.gpu_util import RTOL, assert_close, assert_step_close

pytestmark = pytest.mark.gpu

TABLES = ("xu", "wl", "pb")


@pytest.fixture(scope="module")
def ctx():
    return _lib.context(0)


def _away(v, eps=1e-9):
    v = np.abs(np.asarray(v, np.float64)).reshape(-1)
    v = v[v != 0.0]
    return bool(np.all(np.abs(v - np.round(v)) >= eps)) if v.size else True


def make_problem(seed, n_item, dim, lens, theta=0.5, box=8.0, ctx_max=4, scale=0.5):
    """Random coordinates in a box x box degree square -> the region tree; users with the given train lengths, random targets and
    contexts of 0 .. ctx_max POIs (one position of each user with an empty context, one whose context holds its own target, one
    repeated target when the length allows); one test position per user."""
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.uniform(10, 10 + box, n_item), rng.uniform(-60, -60 + box, n_item)], 1)
    coords[0], coords[1] = (10, -60), (10 + box, -60 + box)
    tree = D.poi2vec_region_tree(coords, theta)
    n_user = len(lens)
    data, tes = {}, {}
    for u, L in enumerate(lens):
        t = rng.integers(0, n_item, L)
        c = [rng.integers(0, n_item, rng.integers(1, ctx_max + 1)) for _ in range(L)]
        if L >= 1:
            c[0] = np.zeros(0, np.int64)
        if L >= 2:
            c[1] = np.append(c[1], t[1])
        if L >= 4:
            t[3] = t[2]
        data[u] = (t, c)
        tes[u] = (rng.integers(0, n_item, 1), [rng.integers(0, n_item, rng.integers(1, ctx_max + 1))])
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    P = dict(xu=f32(rng.uniform(-scale, scale, (n_user, dim))), wl=f32(rng.uniform(-scale, scale, (n_item, dim))),
             pb=f32(rng.uniform(-scale, scale, (tree["n_node"], dim))))
    return dict(P=P, T=tree, data=data, tes=tes, n_user=n_user, n_item=n_item, dim=dim, len_max=max(lens) if len(lens) else 0)


def _margins_ok(pr, users=None):
    for u in (range(pr["n_user"]) if users is None else users):
        t, c = pr["data"][u]
        if len(t) == 0:
            continue
        F = O.forward_terms(pr["P"], pr["T"], u, t, c)
        if not (_away(F["cl"].mean(axis=1)) and _away(F["S"])):
            return False
    return True


def problem(seed, *a, **kw):
    for s in range(seed, seed + 20):
        pr = make_problem(s, *a, **kw)
        if _margins_ok(pr):
            return pr
    raise AssertionError("no seed with margins")


def _csr(side, n_user):
    off, t, coff, c = [0], [], [0], []
    for u in range(n_user):
        tt, cc = side[u]
        for i in range(len(tt)):
            t.append(int(tt[i])); c.extend(int(k) for k in cc[i]); coff.append(len(c))
        off.append(len(t))
    return [np.asarray(x, np.int32) for x in (off, t, coff, c)]


def model_of(pr, alpha=0.01, lam=0.001, **kw):
    tra, tes = _csr(pr["data"], pr["n_user"]), _csr(pr["tes"], pr["n_user"])
    T = pr["T"]
    ds = D.Poi2vecDataset(n_user=pr["n_user"], n_item=pr["n_item"], n_node=T["n_node"], depth=T["depth"], coords=None, off=tra[0], tra_t=tra[1],
                          tra_coff=tra[2], tra_c=tra[3], tes_off=tes[0], tes_t=tes[1], tes_coff=tes[2], tes_c=tes[3], routes=T["routes"],
                          lrs=T["lrs"], probs=T["probs"], rid=T["rid"])
    return OboPoi2vec(ds, None, [alpha, lam], pr["n_user"], pr["n_item"], T["n_node"], pr["dim"], T["probs"], T["routes"], T["lrs"],
                      init=pr["P"], **kw)


def tables(m):
    return dict(xu=m._xu.cpu().numpy().astype(np.float64), wl=m._wl[:m.n_item].cpu().numpy().astype(np.float64),
                pb=m._pb.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("L", [1, 2, 17, 300])
@pytest.mark.parametrize("dim", [4, 20, 64, 128])
def test_one_user_launch_equals_the_reference_step(ctx, dim, L):
    ctx.set_batch_cap(1)
    for n_item in (200, 30000):
        pr = problem(100 + dim + L, n_item, dim, [L, L + 5, L])
        for u in (0, 1):                                       # user 0 is shorter than len_max (padding), user 1 the longest
            m = model_of(pr)
            assert (m._lens[u] < m.len_max) == (u == 0)
            ctx.take_bad_ids()
            loss = m.train(u)
            assert ctx.take_bad_ids() == 0
            Q, ref = O.step(pr["P"], pr["T"], u, *pr["data"][u], 0.01, 0.001, pr["len_max"])
            what = "dim %d L %d n_item %d user %d" % (dim, L, n_item, u)
            print(what, "loss", loss, ref)
            assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref)), (what, loss, ref)
            assert_step_close(tables(m), Q, pr["P"], TABLES, what)
            if u == 0:                                         # the padded bidx writes routes[0]'s nodes back last
                keep = np.unique(pr["T"]["routes"][0])
                np.testing.assert_array_equal(tables(m)["pb"][keep], pr["P"]["pb"][keep])
            assert float(m._wl[m.n_item].abs().max()) == 0.0
            if L >= 17:                                        # (a write through a duplicate route has probs 0 and moves nothing)
                assert np.abs(Q["pb"] - pr["P"]["pb"]).max() > 0


def test_indicator_of_two(ctx):
    """A context whose mean exceeds 1 in magnitude: ind_i = 2, S_i can pass 1 and floor(1 - S_i) turns negative."""
    ctx.set_batch_cap(1)
    pr = problem(7, 120, 20, [3, 6], ctx_max=3)
    big = pr["data"][0][1][1]
    pr["P"]["wl"][big] = np.float32(0.45) + np.float32(0.01) * np.arange(20)[None, :].astype(np.float32)
    pr["data"][0][1][1] = np.concatenate([big, big, big])[:max(3, len(big) * 3)]
    F = O.forward_terms(pr["P"], pr["T"], 0, *pr["data"][0])
    assert F["ind"][1] >= 2 and _margins_ok(pr, [0])
    m = model_of(pr)
    loss = m.train(0)
    Q, ref = O.step(pr["P"], pr["T"], 0, *pr["data"][0], 0.01, 0.001, pr["len_max"])
    assert np.isfinite(ref)                                    # (paths > 0: the ind >= 2 arithmetic is what is compared)
    assert abs(loss - ref) <= RTOL * max(1.0, abs(ref))
    assert_step_close(tables(m), Q, pr["P"], TABLES, "ind 2")


@pytest.mark.parametrize("cap", [1, 64, 1e9])
def test_batched_launch_follows_the_capped_rule(ctx, cap):
    lens = [0, 1, 2, 3, 5, 8, 13, 21, 34, 40, 7, 1, 0, 12, 40, 9, 4, 6, 2, 30]
    pr = problem(31, 300, 20, lens)
    users = np.array([3, 0, 5, 7, 19, 1, 12, 9, 14, 2, 8, 4, 6, 10, 11, 13, 15, 16, 17, 18, 5])      # user 5 twice, users 0 and 12 empty
    ctx.set_batch_cap(cap)
    try:
        m = model_of(pr)
        ctx.take_bad_ids()
        loss = m.train_batch(users)
        Q, ref, M = O.batch_step(pr["P"], pr["T"], users, pr["data"], 0.01, 0.001, pr["len_max"], cap=cap, absmass=True)
        assert ctx.take_bad_ids() + m.rejected == int(np.isnan(ref).sum()) == 2
        assert np.array_equal(np.isnan(loss), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.all(np.abs(loss[ok] - ref[ok]) <= 1e-5 * np.maximum(1.0, np.abs(ref[ok])))
        assert_step_close(tables(m), Q, pr["P"], TABLES, "cap %g" % cap, absmass=M)
    finally:
        ctx.set_batch_cap(1)


def _raw_step(ctx, m, users, n_pos=None, n_ctx=None):
    a = np.asarray(users, np.int64)
    ok = a[(a >= 0) & (a < m.n_user)]
    off, coff = m._tra[0].astype(np.int64), m._tra[2].astype(np.int64)
    n_pos = int(m._lens[ok].sum()) if n_pos is None else n_pos
    n_ctx = int((coff[off[ok + 1]] - coff[off[ok]]).sum()) if n_ctx is None else n_ctx
    uu = torch.as_tensor(a.astype(np.int32)).cuda()
    loss = torch.empty(len(a), dtype=torch.float32, device="cuda")
    P = m._pparams(m._live())
    ctx.check(ctx.lib.poi_poi2vec_step(ctx.handle, ctypes.byref(P), m.off.data_ptr(), m.tgt.data_ptr(), m.coff.data_ptr(), m.cidx.data_ptr(),
                                       uu.data_ptr(), len(a), n_pos, n_ctx, m.len_max, 0.01, 0.001, loss.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return loss.cpu().numpy()


def test_rejection_moves_nothing_and_removal_is_bitwise_equal(ctx):
    lens = [5, 0, 9, 3, 14, 6, 2, 11]
    pr = problem(41, 260, 20, lens)
    ctx.set_batch_cap(64)
    try:
        # alone: an id out of range, an empty user
        for bad in (-1, 8, 1):
            m = model_of(pr)
            ctx.take_bad_ids()
            loss = _raw_step(ctx, m, [bad])
            assert np.isnan(loss[0]) and ctx.take_bad_ids() == 1
            for k in TABLES:
                np.testing.assert_array_equal(tables(m)[k], pr["P"][k])
        # a non-finite loss: user 3's tables make paths <= 0 impossible to force portably, so poison its xu row instead
        good = [4, 0, 2, 7, 5, 6]
        base = model_of(pr)
        l0 = _raw_step(ctx, base, good)
        for bad, poison in ((8, False), (1, False), (3, True)):
            m = model_of(pr)
            if poison:
                m._xu[3] = float("nan")
            ctx.take_bad_ids()
            l1 = _raw_step(ctx, m, good[:3] + [bad] + good[3:])
            assert ctx.take_bad_ids() == 1 and np.isnan(l1[3])
            np.testing.assert_array_equal(np.delete(l1, 3), l0)
            for k in TABLES:
                a, b = tables(m)[k], tables(base)[k]
                if poison and k == "xu":
                    a, b = np.delete(a, 3, 0), np.delete(b, 3, 0)
                np.testing.assert_array_equal(a, b)
        # host totals that do not match: nothing moves, every user rejected
        m = model_of(pr)
        ctx.take_bad_ids()
        l2 = _raw_step(ctx, m, good, n_pos=3)
        assert np.all(np.isnan(l2)) and ctx.take_bad_ids() == len(good)
        for k in TABLES:
            np.testing.assert_array_equal(tables(m)[k], pr["P"][k])
    finally:
        ctx.set_batch_cap(1)


def test_identical_launches_are_bitwise_identical(ctx):
    pr = problem(51, 2000, 64, [30, 12, 1, 45, 45, 7, 19, 3] * 4)
    users = np.random.default_rng(3).permutation(32)
    ctx.set_batch_cap(8)
    try:
        runs = []
        for _ in range(3):
            m = model_of(pr)
            loss = m.train_batch(users)
            runs.append((loss, tables(m)))
        for loss, T in runs[1:]:
            np.testing.assert_array_equal(loss, runs[0][0])
            for k in TABLES:
                np.testing.assert_array_equal(T[k], runs[0][1][k])
    finally:
        ctx.set_batch_cap(1)


def test_one_user_epoch_matches_sequential_oracle_steps(ctx):
    pr = problem(61, 150, 8, [4, 9, 2, 9, 6, 1])
    ctx.set_batch_cap(1)
    m = model_of(pr)
    Q = pr["P"]
    for u in np.random.default_rng(1).permutation(pr["n_user"]):
        loss = m.train(int(u))
        Q, ref = O.step(Q, pr["T"], int(u), *pr["data"][int(u)], 0.01, 0.001, pr["len_max"])
        print("user", u, "loss", loss, ref)
        assert abs(loss - ref) <= RTOL * max(1.0, abs(ref)), (u, loss, ref)
    got = tables(m)
    for k in TABLES:
        assert_close(got[k], Q[k], k)
    assert abs(m.l2.eval() - O.l2(Q, 0.001)) <= 1e-5 * O.l2(Q, 0.001)


def _score_problem(kind):
    if kind == "file":
        import os
        ds = D.load_poi2vec_sequence_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequences_small.txt"))
        rng = np.random.default_rng(5)
        T = dict(routes=ds.routes, lrs=ds.lrs, probs=ds.probs, n_node=ds.n_node)
        return ds, T, rng
    rng = np.random.default_rng(6)
    ds = D.make_poi2vec_synthetic(40, 500, 14, 9, box_km=1500.0, region_threshold=0.1)
    assert ds.n_node >= 2 * 4096 - 1
    return ds, dict(routes=ds.routes, lrs=ds.lrs, probs=ds.probs, n_node=ds.n_node), rng


@pytest.mark.parametrize("eval_context", ["reference", "test"])
@pytest.mark.parametrize("softmax_axis", ["reference", "items"])
@pytest.mark.parametrize("kind", ["file", "box"])
def test_scores_and_topk(ctx, kind, softmax_axis, eval_context):
    ds, T, rng = _score_problem(kind)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    users = np.arange(min(ds.n_user, 11))
    for attempt in range(20):
        P = dict(xu=f32(rng.uniform(-0.5, 0.5, (ds.n_user, 20))), wl=f32(rng.uniform(-0.5, 0.5, (ds.n_item, 20))),
                 pb=f32(rng.uniform(-0.5, 0.5, (ds.n_node, 20))))
        m = OboPoi2vec(ds, None, [0.01, 0.001], ds.n_user, ds.n_item, ds.n_node, 20, ds.probs, ds.routes, ds.lrs, init=P,
                       softmax_axis=softmax_axis, eval_context=eval_context)
        length, rc, flat = m._eval_rows(users)
        rc, flat = rc.cpu().numpy(), flat.cpu().numpy()
        cl = np.stack([O.context_sum(P["wl"], flat[rc[r]:rc[r + 1]]) for r in range(len(users) * length)]).reshape(len(users), length, 20)
        ref, z, S = O.scores_factorised(P, T, users, cl, softmax_axis, return_z=True)
        used = np.unique(ds.routes)
        if _away(z[:, used]) and _away(S):
            break
    else:
        raise AssertionError("no draw with margins")
    m.update_trained_params()
    got = m.compute_sub_all_scores(users)
    assert got.shape == ref.shape == (len(users) * length, ds.n_item)
    assert_close(got, ref, "scores %s %s %s" % (kind, softmax_axis, eval_context))
    idx, sc = m.compute_sub_topk(users, 20, return_scores=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), O.topk_desc(got, 20))
    np.testing.assert_array_equal(sc.cpu().numpy(), np.take_along_axis(got, O.topk_desc(got, 20).astype(np.int64), 1))


def test_reference_context_raises_past_a_users_rows(ctx):
    pr = problem(71, 100, 8, [0, 3])
    m = model_of(pr)
    with pytest.raises(ValueError):
        m.compute_sub_all_scores([0])


def test_train_poi2vec_learns(ctx):
    ds = D.make_poi2vec_synthetic(400, 600, 30, 13, local=0.9, n_nbr=8)
    logs = []
    p = dict(epochs=4, batch=16, latent_size=20, seed=5, batch_size_test=64, softmax_axis="items", eval_context="test")
    model, best, hist = harness.train_poi2vec(ds, p, log=logs.append)
    losses = [h["loss"] for h in hist]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    r20 = [h["recall"][20] for h in hist]
    untrained = harness.poi2vec_model(ds, p)
    untrained.update_trained_params()
    r0 = harness.poi2vec_recall(untrained, ds, p, [20])[20]["recall"]
    print("recall@20 untrained", r0, "epochs", r20, "losses", losses)
    # an untrained model (uniform(-0.5, 0.5) tables) ranks by noise.  Measured on MI355X: untrained recall@20 0.030; after the epochs
    # 0.135, 0.2375, 0.3275, 0.3775 (epoch losses 3193, 2984, 2721, 2496).  The bar: halfway in ratio between the two,
    # sqrt(0.3775 / 0.030) = 3.5 times the untrained model, and rising.
    assert r20[-1] > 3.5 * r0 and r20[-1] > r20[0], (r20, r0)
    assert len(logs) == 4 and "sum_loss" in logs[0]
