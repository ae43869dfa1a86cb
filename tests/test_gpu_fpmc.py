"""FPMC-LR on the device (csrc/fpmc.hip, models.OboFpmc_lr, harness.train_fpmc_lr) against the host restatement of the neighbour sets
(data.fpmc_neighbors_host, itself pinned to the reference by tests/test_fpmc_cpu.py) and the float64 oracle of tests/fpmc_oracle.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import poi_amd
from poi_amd import _lib, data as D, harness
from poi_amd.models import OboFpmc_lr
from tests import fpmc_oracle as F
from tests.gpu_util import RTOL, assert_close, delta_excess

pytestmark = pytest.mark.gpu

P_ = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ctx():
    return _lib.context(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_neighbors(ctx, coords, ud_km):
    xy = torch.as_tensor(np.ascontiguousarray(coords, np.float64)).cuda()
    cphi = torch.as_tensor(D.cos_lat(np.asarray(coords))).cuda()
    order = torch.argsort(xy[:, 0], stable=True).to(torch.int32).contiguous()
    n = len(coords)
    c_ud = D.ud_threshold(ud_km)
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.poi_fpmc_neighbor_counts(ctx.handle, P_(xy), P_(cphi), P_(order), n, c_ud, P_(off), _stream()))
    total = int(off[-1].item())
    nbr = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.poi_fpmc_neighbor_fill(ctx.handle, P_(xy), P_(cphi), P_(order), n, c_ud, P_(off), P_(nbr), _stream()))
    return off.cpu().numpy(), nbr[:total].cpu().numpy(), order.cpu().numpy()


def _check_csr(dev, host, order, exact_order):
    off_d, ids_d, _ = dev
    off_h, ids_h = host
    assert off_d[-1] == off_h[-1], (off_d[-1], off_h[-1])
    assert np.array_equal(off_d, off_h)
    rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
    for r in range(len(off_h) - 1):
        d, h = ids_d[off_d[r]:off_d[r + 1]], ids_h[off_h[r]:off_h[r + 1]]
        assert set(d.tolist()) == set(h.tolist()), r
        if exact_order:
            assert np.array_equal(d, h[np.argsort(rank[h], kind="stable")]), r


@pytest.mark.parametrize("name", ["small", "hard"])
def test_neighbor_build_equals_host_on_golden_sets(ctx, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "fpmc_neighbors.npz"))
    xy, ud = g[name + "_coords"], float(g["ud_km"])
    dev = device_neighbors(ctx, xy, ud)
    _check_csr(dev, (g[name + "_off"], g[name + "_ids"]), dev[2], exact_order=True)
    again = device_neighbors(ctx, xy, ud)
    assert np.array_equal(again[0], dev[0]) and np.array_equal(again[1], dev[1])      # deterministic


def test_neighbor_build_equals_host_on_20k_pois(ctx):
    rng = np.random.default_rng(11)
    n = 20000
    centres = np.stack([40.0 + rng.uniform(0, 2.7, 40), -74.0 + rng.uniform(0, 3.5, 40)], 1)
    k = rng.integers(0, 40, n)
    xy = np.stack([centres[k, 0] + rng.normal(0, 0.15, n), centres[k, 1] + rng.normal(0, 0.2, n)], 1)
    xy[:300] = xy[300:600]                                                           # exact duplicates
    dev = device_neighbors(ctx, xy, 20.0)
    host = D.fpmc_neighbors_host(xy, 20.0, block=512)
    _check_csr(dev, host, dev[2], exact_order=False)


def _sampler(ctx, off, nbr, n_item, pos, seed):
    offt = torch.as_tensor(off).cuda(); nbt = torch.as_tensor(nbr if len(nbr) else np.zeros(1, np.int32)).cuda()
    post = torch.as_tensor(np.asarray(pos, np.int32)).cuda()
    out = torch.empty_like(post)
    ctx.check(ctx.lib.poi_fpmc_sample_negatives(ctx.handle, P_(offt), P_(nbt), n_item, P_(post), post.numel(), seed, P_(out), _stream()))
    return out.cpu().numpy()


def test_sampler_contract(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "fpmc_neighbors.npz"))
    off, ids = g["hard_off"], g["hard_ids"]
    n = len(off) - 1
    cnt = np.diff(off)
    rng = np.random.default_rng(2)
    pos = rng.choice(np.nonzero(cnt > 0)[0], 50000)
    j = _sampler(ctx, off, ids, n, pos, 77)
    for t in range(0, len(pos), 7):
        assert j[t] in set(ids[off[pos[t]]:off[pos[t] + 1]].tolist()) and j[t] != pos[t]
    assert np.array_equal(j, _sampler(ctx, off, ids, n, pos, 77))
    assert not np.array_equal(j, _sampler(ctx, off, ids, n, pos, 78))
    lonely = np.nonzero(cnt == 0)[0]
    bad = np.array(([int(lonely[0])] if lonely.size else []) + [-1, n, n + 5], np.int32)
    assert np.all(_sampler(ctx, off, ids, n, bad, 1) == -1)


def test_sampler_is_uniform_over_a_large_neighbour_set(ctx):
    m = 500                                                                          # POI 0 with 500 neighbours
    off = np.array([0, m] + [m] * m, np.int64)
    ids = np.arange(1, m + 1, dtype=np.int32)
    draws = _sampler(ctx, off, ids, m + 1, np.zeros(250000, np.int32), 12345)
    cnt = np.bincount(draws - 1, minlength=m)
    assert cnt.sum() == 250000 and cnt.min() > 0
    e = 250000 / m
    chi2 = ((cnt - e) ** 2 / e).sum()
    assert chi2 < (m - 1) + 5 * np.sqrt(2 * (m - 1)), chi2                           # df = 499: mean 499, sd 31.6


# ---- step ---------------------------------------------------------------------------------------
def _tables(P):
    return {k: torch.as_tensor(P[k], dtype=torch.float32).cuda().contiguous() for k in F.TABLES}


def _launch(ctx, T, n_user, n_item, dim, u, a, i, j, alpha=0.01, lam=0.001):
    prm = _lib.FpmcParams(*[ctypes.c_void_p(T[k].data_ptr()) for k in ("ui", "iu", "ia", "ai")], n_user, n_item, dim)
    cv = lambda v: torch.as_tensor(np.asarray(v, np.int32)).cuda()
    uu, aa, ii, jj = cv(u), cv(a), cv(i), cv(j)
    loss = torch.empty(len(u), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.poi_fpmc_step(ctx.handle, ctypes.byref(prm), P_(uu), P_(aa), P_(ii), P_(jj), len(u), alpha, lam, P_(loss), _stream()))
    return loss.cpu().numpy()


def _host(T):
    return {k: T[k].cpu().numpy().astype(np.float64) for k in F.TABLES}


@pytest.mark.parametrize("dim", [20, 64, 128])
@pytest.mark.parametrize("a_is_i", [False, True])
def test_single_transition_equals_the_reference_step(ctx, dim, a_is_i):
    ctx.set_batch_cap(1)
    rng = np.random.default_rng(dim)
    P = F.init_tables(rng, 6, 40, dim)
    T = _tables(P)
    P = _host(T)
    u, a, i, j = 4, (7 if a_is_i else 19), 7, 33
    loss = _launch(ctx, T, 6, 40, dim, [u], [a], [i], [j])
    Q, ref = F.step(P, u, a, i, j, 0.01, 0.001)
    assert_close(loss, [ref], "loss")
    got = _host(T)
    for k in F.TABLES:
        assert_close(got[k], Q[k], k)
        ex, _ = delta_excess(got[k], Q[k], P[k])
        assert ex <= 1.0, (k, ex)


@pytest.mark.parametrize("cap", [1.0, 64.0])
def test_batched_launch_on_hot_rows_follows_the_snapshot_rule(ctx, cap):
    rng = np.random.default_rng(int(cap))
    n_user, n_item, dim, n = 50, 200, 20, 20000
    P0 = F.init_tables(rng, n_user, n_item, dim)
    w = 1.0 / np.arange(1, n_item + 1)                                                # Zipf: a few very hot rows
    w /= w.sum()
    u = rng.integers(0, n_user, n)
    a, i = rng.choice(n_item, n, p=w), rng.choice(n_item, n, p=w)
    j = rng.choice(n_item, n, p=w)
    j = np.where(j == i, (j + 1) % n_item, j)
    a[:50] = i[:50]                                                                   # a == i: rows of different tables
    T = _tables(P0)
    P = _host(T)
    ctx.set_batch_cap(cap)
    try:
        loss = _launch(ctx, T, n_user, n_item, dim, u, a, i, j)
        Q, ref, M = F.batch_step(P, u, a, i, j, 0.01, 0.001, cap=cap, absmass=True)
        assert np.all(np.isfinite(loss))
        assert_close(loss, ref, "losses")
        got = _host(T)
        for k in F.TABLES:
            ex, row = delta_excess(got[k], Q[k], P[k], absmass=M[k])
            assert ex <= 1.0, (k, row, ex)
        T2 = _tables(P)                                                               # the same launch again: bitwise the same tables
        _launch(ctx, T2, n_user, n_item, dim, u, a, i, j)
        for k in F.TABLES:
            assert torch.equal(T2[k], T[k]), k
    finally:
        ctx.set_batch_cap(1)


def test_bad_transition_moves_nothing(ctx):
    rng = np.random.default_rng(5)
    n_user, n_item, dim, n = 30, 100, 20, 3000
    P = F.init_tables(rng, n_user, n_item, dim)
    u, a, i = rng.integers(0, n_user, n), rng.integers(0, n_item, n), rng.integers(0, n_item, n)
    j = (i + 1 + rng.integers(0, n_item - 1, n)) % n_item
    ctx.take_bad_ids()
    T_ref = _tables(P)
    _launch(ctx, T_ref, n_user, n_item, dim, u, a, i, j)
    assert ctx.take_bad_ids() == 0
    for what, t in (("u", 1234), ("a", 777), ("i==j", 2000), ("j", 5)):
        uu, aa, ii, jj = (np.insert(v, t, v[t]) for v in (u, a, i, j))
        if what == "u":
            uu[t] = n_user
        elif what == "a":
            aa[t] = -3
        elif what == "j":
            jj[t] = n_item + 1
        else:
            jj[t] = ii[t]
        T = _tables(P)
        loss = _launch(ctx, T, n_user, n_item, dim, uu, aa, ii, jj)
        assert np.isnan(loss[t]) and np.isfinite(np.delete(loss, t)).all()
        assert ctx.take_bad_ids() == 1
        for k in F.TABLES:
            assert torch.equal(T[k], T_ref[k]), (what, k)


# ---- model --------------------------------------------------------------------------------------
def _dataset(seed=0, n_user=300, n_item=150, max_len=20):
    return D.make_synthetic(n_user, n_item, max_len, seed=seed, local=0.8, box_km=40.0)


def _model(ds, dim=20, seed=1, **kw):
    return OboFpmc_lr(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_size=dim, seed=seed,
                      coords=ds.coords, **kw)


def test_model_train_batch_raises_on_bad_ids_and_checks_inputs():
    ds = _dataset()
    m = _model(ds)
    with pytest.raises(IndexError):
        m.train_batch([0, 1], [2, 3], [4, 5], [6, 5])
    with pytest.raises(IndexError):
        m.train_batch([0, ds.n_user], [2, 3], [4, 5], [6, 7])
    m.train_batch([0], [2], [4], [6])                                                 # the counter was cleared
    # a train target without a neighbour (UD too small), a user with an empty train sequence: ValueError before any launch
    with pytest.raises(ValueError):
        _model(ds, ud_km=1e-6)
    tab = ds.shard()
    tab.off = tab.off.copy(); tab.off[1] = tab.off[0]
    with pytest.raises(ValueError):
        OboFpmc_lr(train=tab, test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_size=20, coords=ds.coords)


def test_epoch_transitions_and_train_match_the_reference_order():
    ds = _dataset(n_user=40)
    m = _model(ds)
    order = np.random.default_rng(3).permutation(ds.n_user)
    u, a, i, j = (t.cpu().numpy() for t in m.epoch_transitions(9, order))
    off = ds.off.astype(np.int64)
    want = [(x, ds.tra_p[t - 1], ds.tra_p[t]) for x in order for t in range(off[x] + 1, off[x + 1])]
    assert list(zip(u.tolist(), a.tolist(), i.tolist())) == [tuple(map(int, w)) for w in want]
    no, ni = D.fpmc_neighbors_host(ds.coords, 20.0)
    assert all(j[t] in set(ni[no[i[t]]:no[i[t] + 1]].tolist()) for t in range(len(i)))
    P = {k: getattr(m, k).get_value().astype(np.float64) for k in F.TABLES}
    los = m.train(int(u[0]), int(a[0]), int(i[0]), [int(j[0])])
    Q, ref = F.step(P, int(u[0]), int(a[0]), int(i[0]), int(j[0]), 0.01, 0.001)
    assert abs(los - ref) <= RTOL * max(1.0, abs(ref))
    for k in F.TABLES:
        assert_close(getattr(m, k).get_value(), Q[k], k)
    assert np.isclose(m.l2.eval(), F.l2(Q, 0.001), rtol=1e-6)


def test_scores_topk_and_auc_equal_the_oracle():
    ds = _dataset(seed=4)
    m = _model(ds, dim=64)
    m.resample_test_negatives_device(5)
    P = {k: getattr(m, k).get_value().astype(np.float64) for k in F.TABLES}
    last = m.tra_last_poi.cpu().numpy()
    users = np.arange(ds.n_user)
    ref = F.scores(P, users, last)
    assert_close(m.compute_sub_all_scores(users), ref, "scores", rtol=1e-5)
    idx = m.compute_sub_topk(users, 10).cpu().numpy()
    want = np.argsort(-ref, axis=1, kind="stable")[:, :10]
    for r in range(ds.n_user):
        if not np.array_equal(idx[r], want[r]):                                       # only float32-level near ties may swap
            assert np.allclose(ref[r, idx[r]], ref[r, want[r]], atol=1e-5), r
    tp, tq, tm = (t.cpu().numpy() for t in (m.tes_buys_masks, m.tes_buys_neg_masks, m.tes_masks))
    got = m.compute_sub_auc_preference(users)
    flags = F.auc_preference(P, users, last, tp, tq, tm)
    up = (P["ui"][:, None, :] * (P["iu"][tp] - P["iu"][tq])).sum(2) + (P["ai"][last][:, None, :] * (P["ia"][tp] - P["ia"][tq])).sum(2)
    clear = np.abs(up) > 1e-5
    assert np.array_equal(got[clear], flags[clear])
    # the evaluator takes the model unchanged
    from poi_amd.evaluate import GlobalBest, fun_predict_auc_recall_map_ndcg
    p = dict(at_nums=[5, 10])
    ses = harness.compute_start_end(ds.n_user, 32)
    res = fun_predict_auc_recall_map_ndcg(p, m, GlobalBest([5, 10]), 0, ses, ses, ds.tes_p.reshape(-1, 1), np.ones((ds.n_user, 1), np.int32))
    hits10 = sum(int(ds.tes_p[r] in want[r]) for r in range(ds.n_user))
    assert abs(res["at"][10]["hits"] - hits10) <= 2
    assert np.isclose(res["auc"], got.sum() / ds.n_user)


def test_train_fpmc_lr_end_to_end_learns():
    ds = _dataset(seed=7, n_user=600, n_item=150, max_len=20)
    logs = []
    p = dict(epochs=4, at_nums=[5, 10], alpha=0.05, seed=3, batch=1)
    model, best, hist = harness.train_fpmc_lr(ds, p, log=logs.append)
    assert len(hist) == 4 and len(logs) == 4
    losses = [h["loss"] for h in hist]
    assert all(np.isfinite(losses)) and all(np.isfinite(h["l2"]) for h in hist)
    assert losses[3] > losses[0], losses
    assert hist[3]["recall"][10] > hist[0]["recall"][10], [h["recall"] for h in hist]
    for k in F.TABLES:
        assert np.isfinite(getattr(model, k).get_value()).all()
