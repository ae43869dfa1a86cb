"""-m gpu: VBPR on the device (csrc/vbpr.hip, models.OboVBpr, harness.train_vbpr) against the float64 oracle of tests/vbpr_oracle.py run
from the float32-rounded inputs.  Bars: gpu_util.RTOL on the weights and DELTA_RTOL per row of the update (assert_step_close), no loose
entries.  Two feature regimes throughout: unit-scale features with the reference's init (|x| ~ 12 at F = 1024: the sigmoid is saturated
and g carries the absolute error of x as its relative error) and features scaled by 1 / sqrt(F) (|x| < 4: the ei gradient carries the
result)."""
import numpy as np
import pytest

from tests import vbpr_oracle as V
from tests.gpu_util import RTOL, assert_close, assert_step_close, round_f32, toy_problem
from tests.test_gpu_bpr import _triples
from tests.test_gpu_session import qualifying

pytestmark = pytest.mark.gpu

ALPHA, LAM, LAM_EV = 0.01, 0.001, 0.002
REGIMES = ("unit", "scaled")


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    return poi_amd


def _setup(pa, seed, n_user, n_item, D, F, regime):
    """(toy tables, float32-rounded float64 parameters, float32-rounded float64 features)"""
    T = toy_problem(seed, n_user=n_user, n_item=n_item, dim=D)
    P = round_f32(V.init_params(np.random.default_rng(seed + 7), n_user, n_item, D, F))
    fi = pa.data.synthetic_features(n_item, F, seed + 3, scale=None if regime == "unit" else 1.0 / np.sqrt(F)).astype(np.float64)
    return T, P, fi


def _model(pa, T, P, fi, D, F):
    return pa.models.OboVBpr(train=T["train"], test=T["test"], alpha_lambda=[ALPHA, LAM, LAM_EV, 0.0], n_user=T["n_user"], n_item=T["n_item"],
                             n_in=D, n_hidden=D, n_img=F, fea_img=fi, init=P)


def _state(m):
    return {k: getattr(m, k).get_value() for k in V.NAMES}


def _bits(m):
    import torch
    return [getattr(m, k).t.clone().view(torch.int32) for k in V.NAMES]


# ---- 1: the reference step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("cap", [1.0, 8.0])
@pytest.mark.parametrize("D,F", [(8, 36), (20, 100), (32, 260), (64, 1024)])
def test_single_triple_is_the_reference_step(pa, D, F, cap, regime):
    n_user, n_item = 9, 40
    T, P, fi = _setup(pa, D + F, n_user, n_item, D, F, regime)
    m = _model(pa, T, P, fi, D, F)
    u, p, q = 4, 17, 31
    exp, el = V.step(P, fi, u, p, q, ALPHA, LAM, LAM_EV)
    m.ctx.set_batch_cap(cap)
    try:
        got = m.train(u, [p, q])
    finally:
        m.ctx.set_batch_cap(1.0)
    print("single step D %d F %d cap %g %s: loss %.9g (oracle %.9g)" % (D, F, cap, regime, got, el))
    assert abs(got - el) <= RTOL * max(abs(el), 1e-30)
    assert_step_close(_state(m), exp, P, V.NAMES, "D %d F %d cap %g %s" % (D, F, cap, regime))
    assert np.array_equal(m.fi.get_value(), fi.astype(np.float32))


# ---- 2: the batch rule with shared rows ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_problem(pa):
    D, F, n_user, n_item = 64, 1024, 120, 300
    return {r: _setup(pa, 50, n_user, n_item, D, F, r) for r in REGIMES}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("cap", [1.0, 8.0, 1e9])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 3000])
def test_batch_rule_with_shared_rows(pa, shared_problem, n, cap, regime):
    D, F, n_user, n_item = 64, 1024, 120, 300
    T, P, fi = shared_problem[regime]
    u, p, q = _triples(n, n, n_user, n_item, hot_users=3, hot_items=4)      # hot rows: runs over many 64-touch windows and dense chunks
    exp, el = V.batch_step(P, fi, u, p, q, ALPHA, LAM, LAM_EV, cap)
    x, _, _ = V.margin(P, fi, u, p, q)
    print("n %d cap %g %s: |x| median %.3g max %.3g" % (n, cap, regime, np.median(np.abs(x)), np.abs(x).max()))
    m = _model(pa, T, P, fi, D, F)
    m.ctx.set_batch_cap(cap)
    try:
        got_l = m.train_batch(u, p, q)
    finally:
        m.ctx.set_batch_cap(1.0)
    assert_close(got_l, el, "losses")
    got = _state(m)
    assert_step_close(got, exp, P, V.NAMES, "n %d cap %g %s" % (n, cap, regime))
    for name, rows in (("ux", u), ("ue", u), ("lt", np.concatenate((p, q)))):      # rows no triple touches are bit-identical
        untouched = np.setdiff1d(np.arange(P[name].shape[0]), rows)
        assert np.array_equal(got[name][untouched], np.asarray(P[name], np.float32)[untouched]), name
    assert np.array_equal(m.fi.get_value(), fi.astype(np.float32))


# ---- 3: reproducibility -------------------------------------------------------------------------------------------------------------
def test_identical_launches_are_bitwise_identical_on_any_grid(pa):
    import torch
    D, F, n_user, n_item, n = 64, 1024, 500, 2000, 20000
    T, P, fi = _setup(pa, 51, n_user, n_item, D, F, "scaled")
    u, p, q = _triples(3, n, n_user, n_item, hot_users=5, hot_items=6)
    runs = []
    for grid in (0, 0, 7):
        m = _model(pa, T, P, fi, D, F)
        m.ctx.set_batch_cap(64.0); m.ctx.set_option("vbpr_grid", grid)
        try:
            l = m.train_batch(u, p, q, sync=False)
            m.train_batch(u, p, q, sync=False)      # (a second launch on the moved tables: the workspace is reused)
        finally:
            m.ctx.set_batch_cap(1.0); m.ctx.set_option("vbpr_grid", 0)
        runs.append((_bits(m), l.clone()))
    for bits, l in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], bits))
        assert torch.equal(l.view(torch.int32), runs[0][1].view(torch.int32))
    assert all(torch.isfinite(getattr(m, k).t).all() for k in V.NAMES)
    assert not torch.equal(runs[0][0][3], torch.as_tensor(np.asarray(P["ei"], np.float32)).view(torch.int32).to(runs[0][0][3].device))


# ---- 4: bad ids ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u", "p", "q", "p==q"])
def test_bad_ids_raise_and_move_nothing(pa, kind):
    import torch
    D, F, n_user, n_item, n = 20, 100, 40, 90, 300
    T, P, fi = _setup(pa, 52, n_user, n_item, D, F, "scaled")
    u, p, q = _triples(9, n, n_user, n_item, 5, 9)
    bad_at = [7, 150, 299]
    ub, pb, qb = u.copy(), p.copy(), q.copy()
    for i, j in enumerate(bad_at):
        if kind == "u":
            ub[j] = (n_user, -1, n_user + 5)[i]
        elif kind == "p":
            pb[j] = (n_item + 1, -3, 1 << 20)[i]
        elif kind == "q":
            qb[j] = (n_item + 1, -1, n_item + 2)[i]
        else:
            qb[j] = pb[j]
    keep = np.setdiff1d(np.arange(n), bad_at)
    m = _model(pa, T, P, fi, D, F)
    m.ctx.set_batch_cap(8.0)
    try:
        with pytest.raises(IndexError):
            m.train_batch(ub, pb, qb)
        assert m.ctx.take_bad_ids() == 0                                   # counted once, cleared by the raise
        for k in V.NAMES:
            getattr(m, k).set_value(P[k])
        loss = m.train_batch(ub, pb, qb, sync=False).cpu().numpy()
        assert m.ctx.take_bad_ids() == len(bad_at)
        assert np.isnan(loss[bad_at]).all() and np.isfinite(loss[keep]).all()
        with_bad = _bits(m)
        for k in V.NAMES:
            getattr(m, k).set_value(P[k])
        clean = m.train_batch(u[keep], p[keep], q[keep], sync=False).cpu().numpy()
        assert m.ctx.take_bad_ids() == 0
    finally:
        m.ctx.set_batch_cap(1.0)
    assert all(torch.equal(a, b) for a, b in zip(with_bad, _bits(m)))
    assert np.array_equal(loss[keep].view(np.uint32), clean.view(np.uint32))
    exp, _ = V.batch_step(P, fi, ub, pb, qb, ALPHA, LAM, LAM_EV, 8.0)
    assert_step_close(_state(m), exp, P, V.NAMES, "bad %s" % kind)


# ---- 5: snapshots and scoring -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("U,N,D,F", [(64, 300, 20, 100), (64, 300, 8, 36), (96, 500, 32, 260), (64, 1000, 64, 1024)])
def test_snapshots_scores_auc_and_topk(pa, U, N, D, F, regime):
    K = 20
    for seed in (1, 2, 3):
        T, P, fi = _setup(pa, seed, U, N, D, F, regime)
        m = _model(pa, T, P, fi, D, F)
        u, p, q = _triples(seed, 400, U, N, 5, 9)
        m.ctx.set_batch_cap(8.0)
        try:
            for s in range(0, 400, 100):
                m.train_batch(u[s:s + 100], p[s:s + 100], q[s:s + 100])
        finally:
            m.ctx.set_batch_cap(1.0)
        Pn = {k: v.astype(np.float64) for k, v in _state(m).items()}
        m.update_trained_items(); m.update_trained_users()
        assert m.kdim == 2 * D
        it, us = V.items(Pn, fi), V.users(Pn)
        assert_close(m.trained_items.get_value(), it, "trained_items"); assert_close(m.trained_users.get_value(), us, "trained_users")
        assert_close(m.mi.get_value(), it[:, D:], "mi")
        assert np.isclose(m.l2.eval(), V.l2(Pn, LAM, LAM_EV), rtol=1e-6)
        ids = np.arange(U)
        sc = us @ it[:N].T
        assert_close(m.compute_sub_all_scores(ids), sc, "scores")
        tp, tq = T["test"][0][:, 0], T["test"][2][:, 0]
        margin = sc[ids, tp] - sc[ids, tq]
        auc = m.compute_sub_auc_preference(ids)[:, 0]
        sure = np.abs(margin) > 1e-6 * np.abs(sc).max()
        assert np.array_equal(auc[sure], (margin > 0)[sure])
        ok = qualifying(sc, K)
        print("U %d N %d D %d F %d %s seed %d: %.1f %% of rows qualify" % (U, N, D, F, regime, seed, 100.0 * ok.mean()))
        assert ok.mean() >= 0.95
        top = m.compute_sub_topk(ids, K).cpu().numpy()
        want = np.argsort(-sc, axis=1, kind="stable")[:, :K]
        assert np.array_equal(top[ok], want[ok])


# ---- 6: harness ---------------------------------------------------------------------------------------------------------------------
def test_train_vbpr_learns(pa):
    ds = pa.data.make_synthetic(200, 400, 12, seed=11)
    logs = []
    model, best, hist = pa.harness.train_vbpr(ds, dict(epochs=2, latent_size=20, n_img=100, fea_scale=0.1, launch=256, cap=8.0, alpha=0.05, seed=5),
                                              log=logs.append)
    losses = [h["loss"] for h in hist]
    print(logs)
    assert len(hist) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert model.kdim == 40 and all(np.isfinite(h["auc"]) for h in hist)
