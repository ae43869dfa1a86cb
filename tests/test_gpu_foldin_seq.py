"""-m gpu tests of fold-in for the successive-POI models (csrc/foldin_seq.hip: poi_foldin_terms_fpmc / poi_foldin_terms_prme /
poi_foldin_pair; models.OboFpmc_lr / OboPrme fold_in / recommend_new / rank_new; evaluate.foldin_rank_metrics) against the float64 oracle
of tests/foldin_seq_oracle.py run from the float32-rounded inputs.
Bars: gpu_util.RTOL on the rows and the per-epoch losses, assert_delta_close on what the fold-in changed against its start row; the
terms within RTOL of the oracle's relative to the sum of their absolute terms."""
import ctypes

import numpy as np
import pytest

from tests import foldin_oracle as F
from tests import foldin_seq_oracle as S
from tests import prme_oracle as PO
from tests import rank_oracle as RO
from tests.gpu_util import RTOL, assert_close, assert_delta_close

pytestmark = pytest.mark.gpu

ALPHA, LAM, CW = 0.05, 0.001, 0.2
UPW = 4          # users per wave (FOLDIN_USERS_PER_WAVE)
FORMS = {"dot": S.DOT, "metric": S.METRIC}


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dev(pa):
    import torch
    return pa._lib.context(0), torch.device("cuda", 0)


def ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def subset(P, rows, epochs):
    """The toy restricted to the users `rows`, in that order (the epoch-major arrays re-packed)."""
    off, T = P["off"], P["total"]
    lens = [int(off[r + 1] - off[r]) for r in rows]
    pos = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    em = lambda v: np.concatenate([v[e * T + pos] for e in range(max(epochs, 1))])
    no = np.zeros(len(rows) + 1, np.int64); no[1:] = np.cumsum(lens)
    return dict(P, off=no, p=P["p"][pos], q=em(P["q"]), c=em(P["c"]), a=P["a"][pos], gap=P["gap"][pos], dist=P["dist"][pos], total=len(pos),
                w0=P["w0"][list(rows)], lens=lens)


def raw_chain(pa, P, form, epochs, stride, w0=False, alias=False, rows=None, use_a=True, use_c=True, first=1, alpha=ALPHA, lam=LAM):
    """One poi_foldin_pair call on the toy P (optionally on the users `rows` only) -> (w, loss, bad count) on the host."""
    import torch
    ctx, dev = _dev(pa)
    if rows is not None:
        P = subset(P, rows, epochs)
        stride = P["total"] if stride else 0
    n, dim = len(P["off"]) - 1, P["dim"]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    items = t(P["y"], torch.float32)
    off, p, q = t(P["off"], torch.int32), t(np.append(P["p"], 0), torch.int32), t(np.append(P["q"], 0), torch.int32)
    a = t(np.append(P["a"], 0.0), torch.float64) if use_a else None
    c = t(np.append(P["c"], 0.0), torch.float64) if use_c else None
    wi = t(P["w0"], torch.float32) if w0 else None
    wo = wi if alias else torch.full((n, dim), 7.0, dtype=torch.float32, device=dev)
    loss = torch.full((n, max(epochs, 1)), 7.0, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.poi_foldin_pair(ctx.handle, ptr(items), P["n_item"], dim, form, first, ptr(off), ptr(p), ptr(q), int(stride), ptr(a), ptr(c),
                                      int(stride), n, epochs, alpha, lam, ptr(wi), ptr(wo), ptr(loss), st))
    bad = ctx.take_bad_ids(st.value)
    return wo.cpu().numpy(), loss.cpu().numpy()[:, :epochs], bad


def raw_terms(pa, model, P, epochs, stride, dist=True, cw=CW):
    """One terms launch on the toy -> (a (total) or None, c (n_epoch, total)) on the host; the buffers are pre-filled with 7."""
    import torch
    ctx, dev = _dev(pa)
    L = pa._lib
    n, T, dim = len(P["off"]) - 1, P["total"], P["dim"]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    off, p, q = t(P["off"], torch.int32), t(np.append(P["p"], 0), torch.int32), t(np.append(P["q"], 0), torch.int32)
    ne = epochs if stride else 1
    c = torch.full((ne * T + 1,), 7.0, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    s_, v_ = t(P["s"], torch.float32), t(P["v"], torch.float32)
    if model == "fpmc":
        prm = L.FpmcParams(None, None, ptr(s_), ptr(v_), 1, P["n_item"], dim)
        ctx.check(ctx.lib.poi_foldin_terms_fpmc(ctx.handle, ctypes.byref(prm), ptr(off), ptr(p), ptr(q), int(stride), n, T, epochs, ptr(c), st))
        a = None
    else:
        prm = L.PrmeParams(None, None, ptr(s_), 1, P["n_item"], dim)
        gap, dd, xy = t(np.append(P["gap"], 0), torch.int32), t(np.append(P["dist"], 0.0), torch.float64), t(P["cordi"], torch.float64)
        a = torch.full((T + 1,), 7.0, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.poi_foldin_terms_prme(ctx.handle, ctypes.byref(prm), ptr(xy), ptr(off), ptr(p), ptr(q), int(stride), ptr(gap),
                                                ptr(dd) if dist else None, n, T, epochs, S.THD, cw, ptr(a), ptr(c), st))
        assert float(a[T]) == 7.0
        a = a.cpu().numpy()[:T]
    assert float(c[ne * T]) == 7.0, "the terms pass wrote past its last entry"
    assert ctx.take_bad_ids(st.value) == 0
    return a, c.cpu().numpy()[:ne * T].reshape(ne, T)


def check_chain(P, form, epochs, stride, got, w0, what, **kw):
    W, L = S.chain(form, P["y"], P["off"], P["p"], P["q"], stride, epochs, ALPHA, LAM, P["a"], P["c"], stride, w0, **kw)
    start = np.zeros_like(W) if w0 is None else w0
    e = assert_close(got[0], W, what + " rows")
    assert_delta_close(got[0], W, start, what + " update")
    assert_close(got[1], L, what + " losses")
    assert got[2] == 0
    return e


# ---- 1: the chain against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("dim", [4, 20, 64, 128])
@pytest.mark.parametrize("form", ["dot", "metric"])
def test_chain_parity(pa, form, dim, epochs):
    P = S.toy(100 + dim, dim, [0, 1, 2, 7, 50], epochs)
    assert any(P["p"][i] == P["q"][i] for i in range(P["total"])) and any(P["p"][i] == P["p"][i - 1] for i in range(1, P["total"]))
    f = FORMS[form]
    for stride in (0, P["total"]):
        what = "%s dim %d epochs %d stride %d" % (form, dim, epochs, stride)
        e0 = check_chain(P, f, epochs, stride, raw_chain(pa, P, f, epochs, stride), None, what + " w0 NULL")
        e1 = check_chain(P, f, epochs, stride, raw_chain(pa, P, f, epochs, stride, w0=True), P["w0"], what + " w0")
        print("%s: rel err %.2e (w0 NULL) %.2e (w0)" % (what, e0, e1))
    given, alias = raw_chain(pa, P, f, epochs, P["total"], w0=True), raw_chain(pa, P, f, epochs, P["total"], w0=True, alias=True)
    assert np.array_equal(bits(given[0]), bits(alias[0])) and np.array_equal(bits(given[1]), bits(alias[1])), "w_out aliasing w0 changed the result"
    # lengths 0 and 1 have no transition: the start row and zero losses
    assert np.array_equal(bits(given[0][:2]), bits(P["w0"][:2])) and not given[1][:2].any()
    # a = NULL is 1, c = NULL is 0
    got = raw_chain(pa, P, f, epochs, P["total"], w0=True, use_a=False, use_c=False)
    W, L = S.chain(f, P["y"], P["off"], P["p"], P["q"], P["total"], epochs, ALPHA, LAM, None, None, 0, P["w0"])
    assert_close(got[0], W, "no terms rows"); assert_close(got[1], L, "no terms losses")


@pytest.mark.parametrize("n", [1, UPW - 1, UPW, UPW + 1, 70])
@pytest.mark.parametrize("form", ["dot", "metric"])
def test_group_and_wave_edges(pa, form, n):
    lens = np.random.default_rng(n).integers(0, 13, n)
    lens[0] = 12
    P = S.toy(200 + n, 20, lens, 2)
    check_chain(P, FORMS[form], 2, P["total"], raw_chain(pa, P, FORMS[form], 2, P["total"], w0=True), P["w0"], "%s n %d" % (form, n))


# ---- 2: the terms pass against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 20, 64, 128])
@pytest.mark.parametrize("model", ["fpmc", "prme"])
def test_terms_pass(pa, model, dim):
    epochs = 3
    P = S.toy(600 + dim, dim, [0, 1, 2, 7, 50, 3], epochs)
    assert {S.THD - 1, S.THD, S.THD + 1} <= set(P["gap"].tolist())
    P["q"][int(P["off"][4]) + 5] = -1                                      # a skipped step: c = 0
    T = dict(ia=P["s"], ai=P["v"]) if model == "fpmc" else dict(ds=P["s"])
    worst = 0.0
    for stride in (0, P["total"]):
        a, c = raw_terms(pa, model, P, epochs, stride)
        ref = S.terms(model, T, P["off"], P["p"], P["q"], stride, epochs, P["gap"], P["dist"], None, S.THD, CW)
        assert c.shape == ref["c"].shape and np.isfinite(c).all()
        starts = P["off"][:-1][np.diff(P["off"]) > 0]
        assert not c[:, starts].any() and c[0, int(P["off"][4]) + 5] == 0.0
        err = np.abs(c - ref["c"]) / np.maximum(ref["mass"], 1e-300)
        assert (err[ref["mass"] > 0] <= RTOL).all() and (c[ref["mass"] == 0] == 0).all()
        worst = max(worst, float(err[ref["mass"] > 0].max()))
        if model == "prme":
            assert not a[starts].any()
            ea = np.abs(a - ref["a"]) / np.maximum(np.abs(ref["a"]), 1e-300)
            assert (ea[ref["a"] != 0] <= RTOL).all()
            far = P["gap"] > S.THD
            steps = np.ones(P["total"], bool); steps[starts] = False
            assert (a[far & steps] == 1.0).all() and not c[:, far & steps].any() and (a[(P["gap"] == S.THD) & steps] != 1.0).all()
            worst = max(worst, float(ea.max()))
    print("%s dim %d: worst relative error of the terms %.2e" % (model, dim, worst))
    if model == "prme":
        # dists=None: cal_dis of the coordinates on the device equals explicit cal_dis distances
        xy = P["cordi"]
        d = np.zeros(P["total"])
        d[1:] = PO.cal_dis(xy[P["p"][1:], 0], xy[P["p"][1:], 1], xy[P["p"][:-1], 0], xy[P["p"][:-1], 1])
        a0, c0 = raw_terms(pa, model, P, epochs, P["total"], dist=False)
        a1, c1 = raw_terms(pa, model, dict(P, dist=d), epochs, P["total"])
        ref = S.terms(model, T, P["off"], P["p"], P["q"], P["total"], epochs, P["gap"], None, xy, S.THD, CW)
        assert np.abs(a0 - a1).max() <= 1e-12 * np.abs(a1).max() and np.abs(c0 - c1).max() <= 1e-12 * np.abs(c1).max()
        assert np.abs(a0 - ref["a"]).max() <= RTOL * np.abs(ref["a"]).max()


# ---- 3: the dot form without terms is poi_foldin_bpr ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [20, 128])
def test_dot_form_without_terms_is_foldin_bpr_bit_for_bit(pa, dim):
    from tests.test_gpu_foldin import raw as raw_bpr
    P = S.toy(700 + dim, dim, [0, 1, 2, 7, 50, 12, 3], 3)
    B = dict(P, items=P["y"])
    for stride in (0, P["total"]):
        ours = raw_chain(pa, P, S.DOT, 3, stride, w0=True, use_a=False, use_c=False, first=0)
        bpr = raw_bpr(pa, B, 3, stride, w0=True)
        assert np.array_equal(bits(ours[0]), bits(bpr[0])) and np.array_equal(bits(ours[1]), bits(bpr[1])) and ours[2] == bpr[2] == 0


# ---- 4: independence ----------------------------------------------------------------------------------------------------------------------------
def test_a_users_bits_do_not_depend_on_the_call(pa):
    n = 70
    lens = np.random.default_rng(1).integers(0, 13, n)
    P = S.toy(300, 40, lens, 2)
    for form in (S.DOT, S.METRIC):
        full = raw_chain(pa, P, form, 2, P["total"], w0=True)
        again = raw_chain(pa, P, form, 2, P["total"], w0=True)
        assert np.array_equal(bits(full[0]), bits(again[0])) and np.array_equal(bits(full[1]), bits(again[1])), "identical calls differ"
        perm = np.random.default_rng(2).permutation(n)
        shuf = raw_chain(pa, P, form, 2, P["total"], w0=True, rows=perm)
        assert np.array_equal(bits(shuf[0]), bits(full[0][perm])) and np.array_equal(bits(shuf[1]), bits(full[1][perm])), "a shuffled call differs"
        for r in range(n):
            one = raw_chain(pa, P, form, 2, P["total"], w0=True, rows=[r])
            assert np.array_equal(bits(one[0][0]), bits(full[0][r])) and np.array_equal(bits(one[1][0]), bits(full[1][r])), "user %d alone differs" % r
    # the terms of a position do not depend on the call either
    a, c = raw_terms(pa, "prme", P, 2, P["total"])
    perm = np.random.default_rng(3).permutation(n)
    Q = subset(P, perm, 2)
    a2, c2 = raw_terms(pa, "prme", Q, 2, Q["total"])
    pos = np.concatenate([np.arange(P["off"][r], P["off"][r + 1]) for r in perm]).astype(np.int64)
    assert np.array_equal(a2, a[pos]) and np.array_equal(c2, c[:, pos])


# ---- models --------------------------------------------------------------------------------------------------------------------------------
N_USER = 6


def _train_lists(rng, n_item, n_user=N_USER, length=5, avoid=None):
    """Train sequences over [0, n_item) that never hold the POI `avoid`."""
    return [[int(x) if x != avoid else (int(x) + 1) % n_item for x in rng.integers(0, n_item, length)] for _ in range(n_user)]


def fpmc_model(pa, P, seed=0, ud_km=500.0, avoid=None):
    """An OboFpmc_lr on the toy's tables (iu = y, ia = s, ai = v); every POI neighbours every other (ud_km)."""
    rng = np.random.default_rng(seed)
    N, dim = len(P["y"]) - 1, P["y"].shape[1]
    ui = F.f32(rng.uniform(-0.5, 0.5, (N_USER, dim)))
    tes = [rng.integers(0, N, (N_USER, 1)), np.ones((N_USER, 1), int), rng.integers(0, N, (N_USER, 1))]
    return pa.models.OboFpmc_lr(train=[_train_lists(rng, N, avoid=avoid), None, None], test=tes, alpha_lambda=[0.01, 0.001], n_user=N_USER, n_item=N, n_size=dim,
                                coords=P["cordi"][:N], ud_km=ud_km, init=dict(ui=ui, iu=P["y"], ia=P["s"], ai=P["v"]))


def prme_model(pa, P, seed=0, cw=CW, cls="OboPrme"):
    """An OboPrme on the toy's tables (dp = y, ds = s)."""
    rng = np.random.default_rng(seed)
    N, dim, L = len(P["y"]) - 1, P["y"].shape[1], 5
    du = F.f32(rng.uniform(-0.5, 0.5, (N_USER, dim)))
    pois = np.array(_train_lists(rng, N, length=L))
    one = np.ones((N_USER, L), int)
    train = [pois, rng.integers(1, 500, (N_USER, L)).astype(np.float64), rng.uniform(0, 5, (N_USER, L)), one, rng.integers(0, N, (N_USER, L))]
    test = [rng.integers(0, N, (N_USER, 1)), np.zeros((N_USER, 1)), np.zeros((N_USER, 1)), np.ones((N_USER, 1), int), rng.integers(0, N, (N_USER, 1))]
    return getattr(pa.models, cls)(train=train, test=test, alpha_lambda=[0.01, 0.001], threshold=S.THD, component_weight=cw, cordi=P["cordi"],
                                   n_user=N_USER, n_item=N, n_size=dim, init=dict(du=du, dp=P["y"], ds=P["s"]))


def params_of(m):
    tabs = {k: getattr(m, k).t.clone() for k in m.TABLES}
    if hasattr(m, "_trained"):
        tabs.update({"trained_" + k: v.clone() for k, v in m._trained.items()})
    return tabs


def assert_unchanged(m, before):
    import torch
    assert all(torch.equal(v, before[k]) for k, v in params_of(m).items()), "a fold-in call changed a model parameter"


def hist_of(P):
    return [list(P["p"][P["off"][r]:P["off"][r + 1]]) for r in range(len(P["off"]) - 1)]


def seqs_of(P, key):
    return [list(P[key][P["off"][r]:P["off"][r + 1]]) for r in range(len(P["off"]) - 1)]


# ---- 5: the models' fold_in is the oracle's; one transition is the model's own training step ---------------------------------------------
@pytest.mark.parametrize("model", ["fpmc", "prme"])
def test_model_fold_in_matches_the_oracle(pa, model):
    epochs = 3
    P = S.toy(800, 20, [0, 1, 2, 7, 50, 5], epochs)
    q = P["q"][:epochs * P["total"]]
    if model == "fpmc":
        m = fpmc_model(pa, P)
        before = params_of(m)
        got = m.fold_in(hist_of(P), negatives=q, epochs=epochs, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True)
        W, L = S.fold_in_fpmc(dict(iu=P["y"], ia=P["s"], ai=P["v"]), P["off"], P["p"], P["q"], P["total"], epochs, ALPHA, LAM, P["w0"])
    else:
        m = prme_model(pa, P, cls="OboPRPRM")
        before = params_of(m)
        got = m.fold_in(hist_of(P), seqs_of(P, "gap"), dists=seqs_of(P, "dist"), negatives=q, epochs=epochs, alpha=ALPHA, lam=LAM, init=P["w0"],
                        return_loss=True)
        W, L = S.fold_in_prme(dict(dp=P["y"], ds=P["s"]), P["off"], P["p"], P["q"], P["total"], epochs, ALPHA, LAM, P["gap"], P["dist"], thd=S.THD,
                              cw=CW, w0=P["w0"])
        again = m.fold_in((P["off"], P["p"]), P["gap"], negatives=q, epochs=epochs, alpha=ALPHA, lam=LAM, init=P["w0"])
        Wc, _ = S.fold_in_prme(dict(dp=P["y"], ds=P["s"]), P["off"], P["p"], P["q"], P["total"], epochs, ALPHA, LAM, P["gap"], None, P["cordi"],
                               thd=S.THD, cw=CW, w0=P["w0"])
        assert_close(again.cpu().numpy(), Wc, "rows with dists=None")
        with pytest.raises(ValueError):
            m.fold_in(hist_of(P), P["gap"] + 0.5, negatives=q, epochs=epochs)
    w, loss = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert_close(w, W, model + " rows"); assert_delta_close(w, W, P["w0"], model + " update"); assert_close(loss, L, model + " losses")
    assert_unchanged(m, before)


def test_one_transition_is_the_fpmc_train_step(pa):
    P = S.toy(810, 20, [2], 1)
    m, ref = fpmc_model(pa, P), fpmc_model(pa, P)
    u, a, i, j = 4, 17, 31, 8
    old = m.ui.get_value()[u]
    before = params_of(m)
    w, loss = m.fold_in([[a, i]], negatives=[0, j], epochs=1, init=old[None], return_loss=True)
    assert_unchanged(m, before)
    ref_loss = ref.train(u, a, i, [j])
    new = ref.ui.get_value()[u]
    assert_close(w.cpu().numpy()[0], new, "folded row vs trained ui[u]")
    assert_delta_close(w.cpu().numpy()[0], new, old, "update of ui[u]")
    assert abs(float(loss[0, 0]) + ref_loss) <= RTOL * max(abs(ref_loss), 1e-30)


@pytest.mark.parametrize("gap", [100, S.THD, S.THD + 1])
def test_one_transition_is_the_prme_train_step(pa, gap):
    P = S.toy(820, 20, [2], 1)
    m, ref = prme_model(pa, P), prme_model(pa, P)
    u, prev, p, q, d = 4, 17, 31, 8, 2.5
    old = m.du.get_value()[u]
    before = params_of(m)
    w, loss = m.fold_in([[prev, p]], [[0, gap]], dists=[[0.0, d]], negatives=[0, q], epochs=1, init=old[None], return_loss=True)
    assert_unchanged(m, before)
    ref_loss = ref.train(u, [p, q, prev], d, gap)
    new = ref.du.get_value()[u]
    assert_close(w.cpu().numpy()[0], new, "folded row vs trained du[u]")
    assert_delta_close(w.cpu().numpy()[0], new, old, "update of du[u]")
    assert abs(float(loss[0, 0]) + ref_loss) <= RTOL * max(abs(ref_loss), 1e-30)


# ---- 6: a -1 negative skips its step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dot", "metric"])
def test_a_missing_negative_skips_its_step(pa, form):
    f = FORMS[form]
    P = S.toy(830, 20, [6, 4, 3], 2)
    T = P["total"]
    t = int(P["off"][0]) + 3
    q = P["q"].copy(); q[t] = -1; q[T + t] = -1
    q[P["off"][1] + 1:P["off"][2]] = -1; q[T + P["off"][1] + 1:T + P["off"][2]] = -1      # user 1: nothing but skipped steps
    got = raw_chain(pa, dict(P, q=q), f, 2, T, w0=True)
    assert got[2] == 0
    # user 0 = the history with that check-in's step removed (its a / c go with it)
    keep = np.array([i for i in range(int(P["off"][0]), int(P["off"][1])) if i != t])
    em = lambda v: np.concatenate([v[e * T + keep] for e in range(2)])
    R = dict(P, off=np.array([0, len(keep)]), p=P["p"][keep], q=em(P["q"]), c=em(P["c"]), a=P["a"][keep], total=len(keep), w0=P["w0"][:1])
    ref = raw_chain(pa, R, f, 2, len(keep), w0=True)
    assert np.array_equal(bits(got[0][0]), bits(ref[0][0])) and np.array_equal(bits(got[1][0]), bits(ref[1][0]))
    assert np.array_equal(bits(got[0][1]), bits(P["w0"][1])) and not got[1][1].any(), "a history made of skipped steps must return w0"
    W, L = S.chain(f, P["y"], P["off"], P["p"], q, T, 2, ALPHA, LAM, P["a"], P["c"], T, P["w0"])
    assert_close(got[0], W, "rows"); assert_close(got[1], L, "losses")


def test_the_sampler_marks_a_target_without_neighbours_and_fold_in_skips_it(pa):
    P = S.toy(840, 20, [6, 4], 2)
    xy = P["cordi"].copy()
    lonely = int(P["p"][3])
    xy[lonely] = (10.0, 60.0)                                           # thousands of km from every other POI
    m = fpmc_model(pa, dict(P, cordi=xy), ud_km=100.0, avoid=lonely)      # (the constructor refuses a train target without neighbours)
    import torch
    neg = m.sample_negatives(torch.as_tensor(P["p"].astype(np.int32)), 5).cpu().numpy()
    assert (neg[P["p"] == lonely] == -1).all() and (neg[P["p"] != lonely] >= 0).all()
    w, loss = m.fold_in(hist_of(P), epochs=2, seed=5, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True)
    q = np.concatenate([m.sample_negatives(torch.as_tensor(P["p"].astype(np.int32)), 5 + e).cpu().numpy() for e in range(2)])
    W, L = S.fold_in_fpmc(dict(iu=P["y"], ia=P["s"], ai=P["v"]), P["off"], P["p"], q, P["total"], 2, ALPHA, LAM, P["w0"])
    assert_close(w.cpu().numpy(), W, "rows"); assert_close(loss.cpu().numpy(), L, "losses")


@pytest.mark.parametrize("model", ["fpmc", "prme"])
def test_device_negatives_follow_the_sampler_contract(pa, model):
    P = S.toy(850, 20, [3, 5, 0, 4, 6, 1], 2)
    m = fpmc_model(pa, P) if model == "fpmc" else prme_model(pa, P)
    fold = (lambda **kw: m.fold_in(hist_of(P), **kw)) if model == "fpmc" else (lambda **kw: m.fold_in(hist_of(P), P["gap"], dists=P["dist"], **kw))
    a = fold(epochs=3, seed=11, return_loss=True)
    b = fold(epochs=3, seed=11, return_loss=True)
    c = fold(epochs=3, seed=12)
    assert np.array_equal(bits(a[0].cpu().numpy()), bits(b[0].cpu().numpy())) and not np.array_equal(bits(a[0].cpu().numpy()), bits(c.cpu().numpy()))
    w, loss = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert np.isfinite(w).all() and (loss[[0, 1, 3, 4]] > 0).all() and not w[[2, 5]].any() and not loss[[2, 5]].any()


# ---- 7: bad input ------------------------------------------------------------------------------------------------------------------------------
def test_bad_input_fpmc(pa):
    import torch
    P = S.toy(500, 20, [3, 5, 0, 4, 6, 2], 2)
    m = fpmc_model(pa, P)
    before = params_of(m)
    N, T = P["n_item"], P["total"]
    hist = hist_of(P)
    q2 = P["q"][:2 * T]
    for bad_call, exc in ((lambda: m.fold_in([[1, N + 1]] + hist[1:], epochs=2), IndexError),
                          (lambda: m.fold_in([[1, -1]] + hist[1:], epochs=2), IndexError),
                          (lambda: m.fold_in(hist, negatives=np.append(q2[:-1], N + 1), epochs=2), IndexError),
                          (lambda: m.fold_in(hist, negatives=np.append(q2[:-1], -2), epochs=2), IndexError),
                          (lambda: m.fold_in((P["off"], np.append(P["p"][:-1], N + 1)), epochs=2), IndexError),
                          (lambda: m.fold_in((P["off"][::-1].copy(), P["p"]), epochs=2), ValueError),
                          (lambda: m.fold_in(hist, negatives=q2[:-1], epochs=2), ValueError),
                          (lambda: m.fold_in(hist, epochs=-1), ValueError),
                          (lambda: m.recommend_new(hist, 5, epochs=1), ValueError)):                  # (history 2 is empty: no last POI)
        with pytest.raises(exc):
            bad_call()
        assert m.ctx.take_bad_ids(m._stream().value) == 0, "a host check let a launch through"
    # device tensors: the kernel rejects user 3 alone
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).to(m.device)
    kw = dict(epochs=2, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True)
    good = m.fold_in((dev(P["off"]), dev(P["p"])), negatives=dev(q2), **kw)
    keep = [0, 1, 2, 4, 5]
    for where in ("p", "p first", "q"):
        p_bad, q_bad = P["p"].copy(), q2.copy()
        if where == "p":
            p_bad[P["off"][3] + 1] = N + 1
        elif where == "p first":
            p_bad[P["off"][3]] = -4                              # only ever a prev: the terms pass marks it
        else:
            q_bad[T + P["off"][3] + 2] = -3                      # second epoch
        w, loss = m.fold_in((dev(P["off"]), dev(p_bad)), negatives=dev(q_bad), sync=False, **kw)
        assert m.ctx.take_bad_ids(m._stream().value) == 1, where
        w, loss = w.cpu().numpy(), loss.cpu().numpy()
        assert np.isnan(w[3]).all() and np.isnan(loss[3]).all(), where
        assert np.array_equal(bits(w[keep]), bits(good[0].cpu().numpy()[keep])) and np.array_equal(bits(loss[keep]), bits(good[1].cpu().numpy()[keep]))
        with pytest.raises(IndexError):
            m.fold_in((dev(P["off"]), dev(p_bad)), negatives=dev(q_bad), epochs=2)
    # epochs = 0 returns the init; "zeros" gives zeros; "mean" the mean row of ui
    w = m.fold_in(hist, epochs=0, init=P["w0"]).cpu().numpy()
    assert np.array_equal(bits(w), bits(P["w0"]))
    assert not m.fold_in(hist, epochs=0).cpu().numpy().any()
    mean = m.fold_in(hist, epochs=0, init="mean").cpu().numpy()
    assert np.allclose(mean, m.ui.get_value().mean(0)[None], rtol=1e-6, atol=1e-7)
    assert_unchanged(m, before)


def test_bad_input_prme(pa):
    import torch
    P = S.toy(520, 20, [3, 5, 0, 4, 6, 2], 2)
    m = prme_model(pa, P)
    before = params_of(m)
    N, T = P["n_item"], P["total"]
    hist = hist_of(P)
    q2 = P["q"][:2 * T]
    bad_d = P["dist"].copy(); bad_d[4] = -1.0
    for bad_call, exc in ((lambda: m.fold_in([[1, N + 1]] + hist[1:], P["gap"], epochs=2), IndexError),
                          (lambda: m.fold_in(hist, P["gap"], negatives=np.append(q2[:-1], N + 1), epochs=2), IndexError),
                          (lambda: m.fold_in(hist, P["gap"][:-1], epochs=2), ValueError),
                          (lambda: m.fold_in(hist, P["gap"] + 0.25, epochs=2), ValueError),
                          (lambda: m.fold_in(hist, P["gap"], dists=bad_d, epochs=2), ValueError),
                          (lambda: m.fold_in(hist, P["gap"], dists=np.where(np.arange(T) == 4, np.inf, P["dist"]), epochs=2), ValueError)):
        with pytest.raises(exc):
            bad_call()
        assert m.ctx.take_bad_ids(m._stream().value) == 0, "a host check let a launch through"
    dev = lambda a, dt=torch.int32: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(m.device)
    kw = dict(epochs=2, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True)
    good = m.fold_in((dev(P["off"]), dev(P["p"])), dev(P["gap"]), dists=dev(P["dist"], torch.float64), negatives=dev(q2), **kw)
    keep = [0, 1, 2, 4, 5]
    t3 = int(P["off"][3]) + 1
    cases = [("p", N + 1, None), ("q", -3, None), ("d", None, -0.5), ("d", None, np.inf), ("d", None, np.nan)]
    for where, bad_id, bad_dist in cases:
        p_bad, q_bad, d_bad = P["p"].copy(), q2.copy(), P["dist"].copy()
        if where == "p":
            p_bad[t3] = bad_id
        elif where == "q":
            q_bad[T + t3 + 1] = bad_id
        else:
            d_bad[t3] = bad_dist
        w, loss = m.fold_in((dev(P["off"]), dev(p_bad)), dev(P["gap"]), dists=dev(d_bad, torch.float64), negatives=dev(q_bad), sync=False, **kw)
        assert m.ctx.take_bad_ids(m._stream().value) == 1, (where, bad_id, bad_dist)
        w, loss = w.cpu().numpy(), loss.cpu().numpy()
        assert np.isnan(w[3]).all() and np.isnan(loss[3]).all(), (where, bad_id, bad_dist)
        assert np.array_equal(bits(w[keep]), bits(good[0].cpu().numpy()[keep])) and np.array_equal(bits(loss[keep]), bits(good[1].cpu().numpy()[keep]))
    assert_unchanged(m, before)


def test_descending_offsets_make_a_bad_user(pa):
    """The raw entry: the LAST user's offsets descend (its range overlaps no other history), the others are untouched."""
    P = S.toy(530, 20, [3, 5, 4], 2)
    for form in (S.DOT, S.METRIC):
        good = raw_chain(pa, P, form, 2, P["total"], w0=True)
        off = P["off"].copy(); off[3] = off[2] - 2
        got = raw_chain(pa, dict(P, off=off), form, 2, P["total"], w0=True)
        assert got[2] == 1 and np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all()
        assert np.array_equal(bits(got[0][:2]), bits(good[0][:2])) and np.array_equal(bits(got[1][:2]), bits(good[1][:2]))
    for args in (dict(form=2), dict(first=2), dict(dim=6)):
        with pytest.raises(pa._lib.PoiError):
            bad_args_call(pa, P, **args)


def bad_args_call(pa, P, form=S.DOT, first=1, dim=None):
    import torch
    ctx, dev = _dev(pa)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    items, off, p, q = t(P["y"], torch.float32), t(P["off"], torch.int32), t(P["p"], torch.int32), t(P["q"], torch.int32)
    w = torch.zeros((3, P["dim"]), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.poi_foldin_pair(ctx.handle, ptr(items), P["n_item"], dim or P["dim"], form, first, ptr(off), ptr(p), ptr(q), 0, None, None, 0, 3, 1,
                                      ALPHA, LAM, None, ptr(w), None, None))


# ---- 8: ranking glue -------------------------------------------------------------------------------------------------------------------------
def _glue_inputs(seed, N=50, dim=20, n=33):
    rng = np.random.default_rng(seed)
    P = S.toy(seed, dim, [1] * n, 1, n_item=N)
    hist = [list(rng.integers(0, N, rng.integers(1, 9))) for _ in range(n)]
    hist[5] = list(rng.permutation(N)[:N - 4])                         # leaves 4 candidates: a -1 tail
    total = sum(map(len, hist))
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum([len(h) for h in hist])
    P.update(off=off, p=np.concatenate(hist), total=total, q=rng.integers(0, N, total), gap=rng.choice([5, 200, S.THD, 900], total),
             dist=rng.uniform(0, 20, total), w0=F.f32(rng.uniform(-0.1, 0.1, (n, dim))))
    return P, hist, rng


def _check_lists(idx, scores, hist, k, band, exclude):
    """idx (n, k) against the stable descending sort of the float64 `scores` rows, on the rows whose first k + 1 ranked scores lie more
    than `band` * max|row| apart; returns the number of such rows."""
    n, N = scores.shape
    checked = 0
    for r in range(n):
        s = scores[r].copy()
        if exclude:
            s[np.unique(hist[r])] = -np.inf
        order = np.lexsort((np.arange(N), -s))
        cand = int(np.isfinite(s).sum())
        want = np.where(np.arange(k) < cand, order[:k], -1)
        top = s[order[:min(k + 1, cand)]]
        if len(top) > 1 and np.min(-np.diff(top)) <= band * np.abs(scores[r]).max():
            continue
        checked += 1
        assert np.array_equal(idx[r], want), (r, idx[r], want)
    return checked


@pytest.mark.parametrize("model", ["fpmc", "prme"])
def test_ranking_glue(pa, model):
    import torch
    from poi_amd.evaluate import foldin_rank_metrics
    P, hist, rng = _glue_inputs(6 if model == "fpmc" else 7)
    N, n, k = P["n_item"], len(hist), 5
    last = np.array([h[-1] for h in hist])
    kw = dict(negatives=P["q"], epochs=3, alpha=ALPHA, lam=LAM, init=P["w0"])
    if model == "fpmc":
        m = fpmc_model(pa, P)
        call = lambda f, *a, **b: f(hist, *a, **b, **kw)
        score_of = lambda w: np.concatenate([w, P["v"][last]], 1) @ np.concatenate([P["y"], P["s"]], 1)[:N].T
        band = RO.GAP
    else:
        m = prme_model(pa, P)
        kw.update(dists=P["dist"])
        call = lambda f, *a, **b: f(hist, P["gap"], *a, **b, **kw)
        score_of = lambda w: PO.score_rows(dict(du=w, dp=P["y"], ds=P["s"]), P["cordi"], np.arange(n), last, cw=float(np.float32(CW)))
        band = 2e-5                                                      # two float32 scores, each within 1e-5 relative (test_gpu_prme's bar)
    before = params_of(m)
    w = call(m.fold_in).cpu().numpy().astype(np.float64)
    scores = score_of(w)
    for exclude in ("history", None):
        idx, sc, cnt = call(m.recommend_new, k, exclude=exclude, return_scores=True, return_counts=True)
        idx, sc, cnt = idx.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
        checked = _check_lists(idx, scores, hist, k, band, exclude)
        assert checked >= n // 2, "too few rows with clear gaps: %d" % checked
        for r in range(n):
            seen = set(hist[r]) if exclude else set()
            assert not set(idx[r][idx[r] >= 0]) & seen and cnt[r] == N - len(seen)
            ok = idx[r] >= 0
            assert np.abs(sc[r][ok] - scores[r][idx[r][ok]]).max() <= 1e-5 * np.abs(scores[r]).max()
        if exclude:
            assert (idx[5][:4] >= 0).all() and (idx[5][4:] == -1).all()
    if model == "fpmc":                                                  # the paper's protocol: candidates within UD of the last check-in
        near = m.recommend_new(hist, k, within_km=8.0, **kw).cpu().numpy()
        d = PO.cal_dis(P["cordi"][last, 0][:, None], P["cordi"][last, 1][:, None], P["cordi"][None, :N, 0], P["cordi"][None, :N, 1])
        for r in range(n):
            got = near[r][near[r] >= 0]
            assert (d[r][got] <= 8.0).all() and not set(got) & set(hist[r])
        assert (near == -1).any()
    # ranks against the oracle on the folded rows
    tgt = np.stack([rng.choice(N, 3, replace=False) for _ in range(n)]).astype(np.int32)
    tm = np.ones_like(tgt); tm[::4, 2] = 0
    eoff = np.zeros(n + 1, np.int32); eoff[1:] = np.cumsum([len(set(h)) for h in hist])
    ex = np.concatenate([np.unique(h) for h in hist]).astype(np.int32)
    for exclude, e in (("history", (eoff, ex)), (None, (None, None))):
        orc = RO.ranks(scores, tgt, tm, e[0], e[1])
        rank, rcnt = call(m.rank_new, (tgt, tm), exclude=exclude, return_counts=True)
        rank = rank.cpu().numpy()
        assert np.array_equal(rank >= 0, orc["rank"] >= 0) and np.array_equal(rcnt.cpu().numpy(), orc["count"])
        keep = RO.exclusion_mask(n, N, e[0], e[1])
        clear = 0
        for r in range(n):
            for i in range(3):
                if orc["rank"][r, i] < 0:
                    continue
                t = tgt[r, i]
                others = keep[r] & (np.arange(N) != t)
                nearby = others & (np.abs(scores[r] - scores[r, t]) <= band * np.abs(scores[r]).max())
                above = int((others & ~nearby & (scores[r] > scores[r, t])).sum())
                assert above <= rank[r, i] <= above + int(nearby.sum()), (r, i)
                if not nearby.any():
                    clear += 1
                    assert rank[r, i] == orc["rank"][r, i]
        assert clear >= 0.9 * (orc["rank"] >= 0).sum()
    extra = dict(gaps=P["gap"]) if model == "prme" else {}
    got = foldin_rank_metrics(m, hist, (tgt, tm), [1, 5, N], exclude=None, **extra, **kw)
    ref = RO.summary(rank, rcnt.cpu().numpy())
    assert set(got) == {"n", "mrr", "mean_rank", "median_rank", "auc_full", "at"} and set(got["at"][5]) == {"hits", "recall", "ndcg"}
    assert got["n"] == (rank >= 0).sum() and got["at"][N]["recall"] == 1.0
    for key in ("mrr", "auc_full", "mean_rank"):
        assert abs(got[key] - ref[key]) < 1e-12, key
    assert got["at"][5]["hits"] == ((rank >= 0) & (rank < 5)).sum()
    assert_unchanged(m, before)


# ---- 9: it learns --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fpmc", "prme"])
def test_it_learns(pa, model):
    """tests/test_foldin_seq_cpu.py shows that the rules themselves meet both conditions on these inputs."""
    from tests.test_foldin_seq_cpu import learn_oracle
    c, P = S.LEARN, S.learn_problem()
    hist = [list(h) for h in P["hist"]]
    kw = dict(negatives=P["q"], alpha=c["alpha"], lam=c["lam"], init=P["w0"])
    if model == "fpmc":
        m = fpmc_model(pa, P)
        call = lambda f, *a, **b: f(hist, *a, **b, **kw)
    else:
        m = prme_model(pa, P, cw=c["cw"])
        kw.update(dists=P["dist"])
        call = lambda f, *a, **b: f(hist, P["gap"], *a, **b, **kw)
    before = params_of(m)
    w, loss = call(m.fold_in, epochs=c["epochs"], return_loss=True)
    loss = loss.cpu().numpy().astype(np.float64)
    W, L = learn_oracle(model, P)
    assert_close(w.cpu().numpy(), W, "rows"); assert_close(loss, L, "losses")
    assert loss[:, -1].mean() < loss[:, 0].mean()
    tgt = P["hist"][:, 1:].astype(np.int32)
    r0 = call(m.rank_new, tgt, exclude=None, epochs=0).cpu().numpy()
    r1 = call(m.rank_new, tgt, exclude=None, epochs=c["epochs"]).cpu().numpy()
    print("%s: epoch losses %s, mean rank %.1f -> %.1f" % (model, np.round(loss.sum(0), 2), r0.mean(), r1.mean()))
    assert (r0 >= 0).all() and (r1 >= 0).all() and r1.mean() < r0.mean()
    assert_unchanged(m, before)
