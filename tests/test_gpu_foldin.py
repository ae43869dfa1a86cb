"""-m gpu tests of fold-in (csrc/foldin.hip, poi_foldin_bpr; models.MfBasic.fold_in / recommend_new / rank_new,
evaluate.foldin_rank_metrics) against the float64 oracle of tests/foldin_oracle.py run from the float32-rounded inputs.
Bars: gpu_util.RTOL on the rows and the per-epoch losses, assert_delta_close on what the fold-in changed against its start row."""
import ctypes

import numpy as np
import pytest

from tests import foldin_oracle as F
from tests import rank_oracle as RO
from tests.gpu_util import RTOL, assert_close, assert_delta_close, toy_problem

pytestmark = pytest.mark.gpu

ALPHA, LAM = 0.05, 0.001
UPW = 4          # users per wave (FOLDIN_USERS_PER_WAVE)


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def raw(pa, P, epochs, stride, w0=False, alias=False, half=False, rows=None, alpha=ALPHA, lam=LAM):
    """One poi_foldin_bpr call on the toy P (optionally on the users `rows` only) -> (w, loss, bad count) on the host."""
    import torch
    ctx = pa._lib.context(0)
    dev = torch.device("cuda", 0)
    if rows is not None:
        P = subset(P, rows, epochs)
        stride = P["total"] if stride else 0
    n, dim = len(P["off"]) - 1, P["dim"]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    items = t(P["items"], torch.float16 if half else torch.float32)
    off, p, q = t(P["off"], torch.int32), t(np.append(P["p"], 0), torch.int32), t(np.append(P["q"], 0), torch.int32)
    wi = t(P["w0"], torch.float32) if w0 else None
    wo = wi if alias else torch.full((n, dim), 7.0, dtype=torch.float32, device=dev)
    loss = torch.full((n, max(epochs, 1)), 7.0, dtype=torch.float32, device=dev)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if half:
        ctx.register_f16(items)
    try:
        ctx.check(ctx.lib.poi_foldin_bpr(ctx.handle, ptr(items), P["n_item"], dim, ptr(off), ptr(p), ptr(q), int(stride), n, epochs, alpha, lam,
                                         ptr(wi), ptr(wo), ptr(loss), st))
        bad = ctx.take_bad_ids(st.value)
    finally:
        if half:
            ctx.unregister_f16(items)
    return wo.cpu().numpy(), loss.cpu().numpy()[:, :epochs], bad


def subset(P, rows, epochs):
    """The toy restricted to the users `rows`, in that order (epoch-major negatives re-packed)."""
    off, T = P["off"], P["total"]
    lens = [int(off[r + 1] - off[r]) for r in rows]
    pos = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    q = np.concatenate([P["q"][e * T + pos] for e in range(max(epochs, 1))])
    no = np.zeros(len(rows) + 1, np.int64); no[1:] = np.cumsum(lens)
    return dict(P, off=no, p=P["p"][pos], q=q, total=len(pos), w0=P["w0"][list(rows)], lens=lens)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(P, epochs, stride, got, w0, what, items=None):
    W, L = F.fold_in(P["items"] if items is None else items, P["off"], P["p"], P["q"], stride, epochs, ALPHA, LAM, w0)
    start = np.zeros_like(W) if w0 is None else w0
    e = assert_close(got[0], W, what + " rows")
    assert_delta_close(got[0], W, start, what + " update")
    assert_close(got[1], L, what + " losses")
    assert got[2] == 0
    return e


# ---- 1: oracle parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("dim", [8, 20, 40, 64, 128, 256])
def test_oracle_parity(pa, dim, epochs):
    P = F.toy(100 + dim, dim, [0, 1, 2, 7, 50], epochs)
    assert any(P["p"][i] == P["q"][i] for i in range(P["total"]))
    for stride in (0, P["total"]):
        what = "dim %d epochs %d stride %d" % (dim, epochs, stride)
        e0 = check(P, epochs, stride, raw(pa, P, epochs, stride), None, what + " w0 NULL")
        e1 = check(P, epochs, stride, raw(pa, P, epochs, stride, w0=True), P["w0"], what + " w0")
        print("%s: rel err %.2e (w0 NULL) %.2e (w0)" % (what, e0, e1))
    given, alias = raw(pa, P, epochs, P["total"], w0=True), raw(pa, P, epochs, P["total"], w0=True, alias=True)
    assert np.array_equal(bits(given[0]), bits(alias[0])) and np.array_equal(bits(given[1]), bits(alias[1])), "w_out aliasing w0 changed the result"
    half = P["items"].astype(np.float16).astype(np.float64)
    check(P, epochs, P["total"], raw(pa, P, epochs, P["total"], w0=True, half=True), P["w0"], "half table", items=half)


# ---- 2: group and wave edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, UPW - 1, UPW, UPW + 1, 70])
def test_group_and_wave_edges(pa, n):
    lens = np.random.default_rng(n).integers(0, 13, n)
    lens[0] = 12
    P = F.toy(200 + n, 20, lens, 2)
    check(P, 2, P["total"], raw(pa, P, 2, P["total"], w0=True), P["w0"], "n %d" % n)


# ---- 3: independence ------------------------------------------------------------------------------------------------------------------------
def test_a_users_bits_do_not_depend_on_the_call(pa):
    n = 70
    lens = np.random.default_rng(1).integers(0, 13, n)
    P = F.toy(300, 40, lens, 2)
    full = raw(pa, P, 2, P["total"], w0=True)
    again = raw(pa, P, 2, P["total"], w0=True)
    assert np.array_equal(bits(full[0]), bits(again[0])) and np.array_equal(bits(full[1]), bits(again[1])), "identical calls differ"
    perm = np.random.default_rng(2).permutation(n)
    shuf = raw(pa, P, 2, P["total"], w0=True, rows=perm)
    assert np.array_equal(bits(shuf[0]), bits(full[0][perm])) and np.array_equal(bits(shuf[1]), bits(full[1][perm])), "a shuffled call differs"
    for r in range(n):
        one = raw(pa, P, 2, P["total"], w0=True, rows=[r])
        assert np.array_equal(bits(one[0][0]), bits(full[0][r])) and np.array_equal(bits(one[1][0]), bits(full[1][r])), "user %d alone differs" % r


# ---- 4: one check-in is the reference step ----------------------------------------------------------------------------------------------
def bpr_model(pa, items, n_user=6, seed=0, **kw):
    n_item, dim = items.shape[0] - 1, items.shape[1]
    T = toy_problem(seed, n_user=n_user, n_item=n_item, dim=dim)
    ux = F.f32(np.random.default_rng(seed + 5).uniform(-0.5, 0.5, (n_user, dim)))
    m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=n_user, n_item=n_item, n_in=dim, n_hidden=dim,
                         init=dict(ux=ux, lt=items), **kw)
    m.update_trained_items(); m.update_trained_users()
    return m


@pytest.mark.parametrize("dim", [8, 64])
def test_one_check_in_is_the_bpr_step(pa, dim):
    P = F.toy(400 + dim, dim, [1], 1)
    m = bpr_model(pa, P["items"])
    u, p, q = 4, 17, 31
    ux = m.ux.get_value()
    w, loss = m.fold_in([[p]], negatives=[q], epochs=1, init=ux[u][None], return_loss=True)
    ref_loss = m.train(u, [p, q])
    new = m.ux.get_value()
    assert_close(w.cpu().numpy()[0], new[u], "folded row vs trained ux[u]")
    assert_delta_close(w.cpu().numpy()[0], new[u], ux[u], "update of ux[u]")
    assert abs(float(loss[0, 0]) - ref_loss) <= RTOL * max(abs(ref_loss), 1e-30)


def test_one_check_in_is_the_vbpr_step(pa):
    from tests.test_gpu_vbpr import _model, _setup
    D, Fi = 8, 36
    T, Pv, fi = _setup(pa, 44, 9, 40, D, Fi, "scaled")
    m = _model(pa, T, Pv, fi, D, Fi)
    m.update_trained_items(); m.update_trained_users()
    u, p, q = 4, 17, 31
    old = m.trained_users.get_value()[u]
    w = m.fold_in([[p]], negatives=[q], epochs=1, init=old[None]).cpu().numpy()[0]
    m.train(u, [p, q])
    new = np.concatenate([m.ux.get_value()[u], m.ue.get_value()[u]])
    assert w.shape == (2 * D,)
    assert_close(w, new, "folded row vs trained [ux[u] | ue[u]]")
    assert_delta_close(w, new, old, "update of [ux[u] | ue[u]]")


# ---- 5: bad input ------------------------------------------------------------------------------------------------------------------------------
def test_bad_input(pa):
    import torch
    P = F.toy(500, 20, [3, 5, 0, 4, 6, 2], 2)
    m = bpr_model(pa, P["items"])
    N = P["n_item"]
    hist = [list(P["p"][P["off"][r]:P["off"][r + 1]]) for r in range(6)]
    q2 = P["q"][:2 * P["total"]]
    for bad_call in (lambda: m.fold_in([[1, N + 1]] + hist[1:], epochs=2),
                     lambda: m.fold_in([[1, -1]] + hist[1:], epochs=2),
                     lambda: m.fold_in(hist, negatives=np.append(q2[:-1], N + 1), epochs=2),
                     lambda: m.fold_in((P["off"], np.append(P["p"][:-1], N + 1)), epochs=2)):
        with pytest.raises(IndexError):
            bad_call()
        assert m.ctx.take_bad_ids(m._stream().value) == 0, "a host check let a launch through"
    # device tensors: the kernel rejects user 3 alone
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).to(m.device)
    good = m.fold_in((dev(P["off"]), dev(P["p"])), negatives=dev(q2), epochs=2, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True)
    for where in ("p", "q"):
        p_bad, q_bad = P["p"].copy(), q2.copy()
        if where == "p":
            p_bad[P["off"][3] + 1] = N + 1
        else:
            q_bad[P["total"] + P["off"][3] + 2] = -3          # second epoch
        w, loss = m.fold_in((dev(P["off"]), dev(p_bad)), negatives=dev(q_bad), epochs=2, alpha=ALPHA, lam=LAM, init=P["w0"], return_loss=True, sync=False)
        assert m.ctx.take_bad_ids(m._stream().value) == 1
        w, loss = w.cpu().numpy(), loss.cpu().numpy()
        assert np.isnan(w[3]).all() and np.isnan(loss[3]).all()
        keep = [0, 1, 2, 4, 5]
        assert np.array_equal(bits(w[keep]), bits(good[0].cpu().numpy()[keep])) and np.array_equal(bits(loss[keep]), bits(good[1].cpu().numpy()[keep]))
        without = raw(pa, P, 2, P["total"], w0=True, rows=keep)
        assert np.array_equal(bits(w[keep]), bits(without[0])), "the other users' bits changed"
        with pytest.raises(IndexError):
            m.fold_in((dev(P["off"]), dev(p_bad)), negatives=dev(q_bad), epochs=2)
    # epochs = 0 returns the init; "zeros" gives zeros
    w = m.fold_in(hist, epochs=0, init=P["w0"]).cpu().numpy()
    assert np.array_equal(bits(w), bits(P["w0"]))
    assert not m.fold_in(hist, epochs=0).cpu().numpy().any()
    mean = m.fold_in(hist, epochs=0, init="mean").cpu().numpy()
    assert np.allclose(mean, m.trained_users.get_value().mean(0)[None], rtol=1e-6, atol=1e-7)


def test_device_negatives_follow_the_sampler_contract(pa):
    P = F.toy(510, 20, [3, 5, 0, 4, 6, 2], 2)
    m = bpr_model(pa, P["items"])
    hist = [list(P["p"][P["off"][r]:P["off"][r + 1]]) for r in range(6)]
    a = m.fold_in(hist, epochs=3, seed=11, return_loss=True)
    b = m.fold_in(hist, epochs=3, seed=11, return_loss=True)
    c = m.fold_in(hist, epochs=3, seed=12)
    assert np.array_equal(bits(a[0].cpu().numpy()), bits(b[0].cpu().numpy())) and not np.array_equal(bits(a[0].cpu().numpy()), bits(c.cpu().numpy()))
    w, loss = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert np.isfinite(w).all() and (loss[[0, 1, 3, 4, 5]] > 0).all() and not w[2].any() and not loss[2].any()


# ---- 6: ranking glue -----------------------------------------------------------------------------------------------------------------------------
def test_ranking_glue(pa):
    import torch
    from poi_amd.evaluate import foldin_rank_metrics
    rng = np.random.default_rng(6)
    N, dim, n, k = 50, 20, 33, 10
    items = F.f32(rng.uniform(-0.5, 0.5, (N + 1, dim)))
    m = bpr_model(pa, items)
    hist = [list(rng.integers(0, N, rng.integers(1, 9))) for _ in range(n)]
    hist[5] = list(rng.permutation(N)[:N - 4])                         # leaves 4 candidates: a -1 tail
    hist[7] = []                                                      # an empty history: the start row ranks
    total = sum(map(len, hist))
    neg = rng.integers(0, N, total)
    kw = dict(negatives=neg, epochs=3, alpha=ALPHA, lam=LAM, init=F.f32(rng.uniform(-0.1, 0.1, (n, dim))))
    w = m.fold_in(hist, **kw)
    idx, sc, cnt = m.recommend_new(hist, k, return_scores=True, return_counts=True, **kw)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(set(h)) for h in hist])
    ex = np.concatenate([np.unique(h) for h in hist if len(h)]).astype(np.int32)
    dev = lambda a: torch.as_tensor(a).to(m.device)
    ref = m._near_launch(w, m.trained_items.t, None, float("inf"), (dev(off), dev(ex)), None, k, True, True, True)
    assert all(torch.equal(a, b) for a, b in zip((idx, sc, cnt), ref)), "recommend_new != _near_launch on the folded rows"
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for r in range(n):
        assert not set(idx[r][idx[r] >= 0]) & set(hist[r]) and cnt[r] == N - len(set(hist[r]))
    assert (idx[5][:4] >= 0).all() and (idx[5][4:] == -1).all() and (idx[7] >= 0).all()
    # a radius around the last check-in
    coords = np.stack((30.0 + rng.uniform(0, 0.3, N), 120.0 + rng.uniform(0, 0.3, N)), axis=1)
    m.set_coords(coords)
    near = m.recommend_new(hist, k, within_km=8.0, **kw)
    last = np.array([h[-1] if len(h) else -1 for h in hist], np.int32)
    ref = m._near_launch(w, m.trained_items.t, dev(last), m._near_radius(8.0), (dev(off), dev(ex)), None, k, False, False, True)
    assert torch.equal(near, ref) and (near.cpu().numpy() == -1).any() and (near.cpu().numpy()[7] >= 0).all()
    # ranks against the oracle on the folded rows
    scores = w.cpu().numpy().astype(np.float64) @ items[:N].T
    tgt = np.stack([rng.choice(N, 3, replace=False) for _ in range(n)]).astype(np.int32)
    tm = np.ones_like(tgt); tm[::4, 2] = 0
    for exclude, e in (("history", (off, ex)), (None, (None, None))):
        orc = RO.ranks(scores, tgt, tm, e[0], e[1])
        rank, rcnt = m.rank_new(hist, (tgt, tm), exclude=exclude, return_counts=True, **kw)
        rank = rank.cpu().numpy()
        assert np.array_equal(rank >= 0, orc["rank"] >= 0) and np.array_equal(rcnt.cpu().numpy(), orc["count"])
        clear = (orc["rank"] >= 0) & (orc["a"] == 0)
        assert clear.sum() >= 0.95 * (orc["rank"] >= 0).sum() and np.array_equal(rank[clear], orc["rank"][clear])
    got = foldin_rank_metrics(m, hist, (tgt, tm), [1, 5, N], exclude=None, **kw)
    ref = RO.summary(rank, rcnt.cpu().numpy())
    assert got["n"] == (rank >= 0).sum() and got["at"][N]["recall"] == 1.0
    for key in ("mrr", "auc_full", "mean_rank"):
        assert abs(got[key] - ref[key]) < 1e-12, key
    assert got["at"][5]["hits"] == ((rank >= 0) & (rank < 5)).sum()


# ---- 7: it learns ----------------------------------------------------------------------------------------------------------------------------------
def test_it_learns(pa):
    """tests/test_foldin_cpu.py shows that the rule itself meets both conditions on these inputs."""
    c, P = F.LEARN, F.learn_problem()
    m = bpr_model(pa, P["items"])
    hist = [list(h) for h in P["hist"]]
    kw = dict(negatives=P["q"], alpha=c["alpha"], lam=c["lam"], init=P["w0"])
    w, loss = m.fold_in(hist, epochs=c["epochs"], return_loss=True, **kw)
    loss = loss.cpu().numpy().astype(np.float64)
    W, L = F.fold_in(P["items"], P["off"], P["p"], P["q"], 0, c["epochs"], c["alpha"], c["lam"], P["w0"])
    assert_close(w.cpu().numpy(), W, "rows"); assert_close(loss, L, "losses")
    assert loss[:, -1].sum() < loss[:, 0].sum()
    before = m.rank_new(hist, P["hist"].astype(np.int32), exclude=None, epochs=0, **kw).cpu().numpy()
    after = m.rank_new(hist, P["hist"].astype(np.int32), exclude=None, epochs=c["epochs"], **kw).cpu().numpy()
    print("epoch losses %s, mean rank %.1f -> %.1f" % (np.round(loss.sum(0), 2), before.mean(), after.mean()))
    assert (before >= 0).all() and (after >= 0).all() and after.mean() < before.mean()
