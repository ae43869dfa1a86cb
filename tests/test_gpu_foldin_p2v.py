"""POI2Vec fold-in on the device (csrc/foldin_p2v.hip, poi_poi2vec_topk_ex; models.OboPoi2vec fold_in / score_new / recommend_new /
rank_new; evaluate.foldin_rank_metrics) against the float64 oracle of tests/foldin_p2v_oracle.py run from the float32-rounded inputs.

Bars: the project's standing ones - rows within RTOL of the oracle in max norm, the update within DELTA_RTOL per row
(assert_delta_close against w0), losses within 1e-5 relative.  The arithmetic is float64 end to end and rounded once, so the kernel
sits near one float32 ulp (DESIGN.md section 22 records the observed maximum); the bars are not tightened here.
The shapes are the smallest at which each mechanism can go wrong - tiles of 16 users and 16 items, staged tiles of 32 items, spans of
P2V_FOLD_SPAN items, workgroups of 64 users - not the workload's."""
import ctypes

import numpy as np
import pytest
import torch

from poi_amd import _lib, data as D, evaluate as E, harness
from tests import foldin_p2v_oracle as FO
from tests import poi2vec_oracle as PO
from tests import rank_oracle as RO
from tests.gpu_util import RTOL, assert_close, assert_delta_close
from tests.test_gpu_poi2vec import model_of, problem, tables

pytestmark = pytest.mark.gpu

SPAN = _lib.P2V_FOLD_SPAN
ALPHA, LAM = 0.1, 0.001


@pytest.fixture(scope="module")
def ctx():
    return _lib.context(0)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_case(seed, n_item, dim, n, l_max=12):
    """wl under the reference's init, n histories of 1 .. l_max check-ins (each of 4 or more repeats one target), w0 uniform."""
    rng = np.random.default_rng(seed)
    wl = f32(rng.uniform(-0.5, 0.5, (n_item, dim)))
    hist = []
    for r in range(n):
        h = rng.integers(0, n_item, 1 + r % l_max)
        if len(h) >= 4:
            h[3] = h[1]
        hist.append(h)
    return wl, hist, f32(rng.uniform(-0.5, 0.5, (n, dim)))


def csr(hist):
    off = np.zeros(len(hist) + 1, np.int32)
    off[1:] = np.cumsum([len(h) for h in hist])
    flat = np.concatenate([np.asarray(h, np.int64) for h in hist]) if len(hist) else np.zeros(0, np.int64)
    return off, (flat if flat.size else np.zeros(1, np.int64)).astype(np.int32)


def raw_fold(ctx, wl, off, tgt, epochs, w0=None, alpha=ALPHA, lam=LAM, pad_row=100.0, in_place=False):
    """poi_foldin_p2v itself.  The table carries one more row (the pad row of the model's wl) filled with `pad_row`: it must not
    enter the softmax."""
    n_item, dim = wl.shape
    n = len(off) - 1
    dev = lambda a, t: torch.as_tensor(np.ascontiguousarray(a, dtype=t)).cuda()
    wld = dev(np.concatenate([wl, np.full((1, dim), pad_row)]), np.float32)
    offd, tgtd = dev(off, np.int32), dev(tgt, np.int32)
    w0d = dev(w0, np.float32) if w0 is not None else None
    out = w0d if in_place else torch.empty((n, dim), dtype=torch.float32, device="cuda")
    loss = torch.full((n, epochs), 7.0, dtype=torch.float32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ctx.check(ctx.lib.poi_foldin_p2v(ctx.handle, ptr(wld), n_item, dim, ptr(offd), ptr(tgtd), n, epochs, alpha, lam, ptr(w0d), ptr(out), ptr(loss),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy()


def check_against_oracle(ctx, wl, hist, w0, epochs, what):
    off, flat = csr(hist)
    ctx.take_bad_ids()
    W, loss = raw_fold(ctx, wl, off, flat, epochs, w0)
    assert ctx.take_bad_ids() == 0
    ref, rl = FO.fold_in(wl, hist, epochs, ALPHA, LAM, w0)
    start = w0 if w0 is not None else np.zeros_like(ref)
    e = assert_close(W, ref, "rows " + what)
    assert_delta_close(W, ref, start, "rows " + what)
    le = float(np.max(np.abs(loss - rl) / np.maximum(1.0, np.abs(rl)))) if rl.size else 0.0
    print("%s: rows %.2e of max|row|, losses %.2e relative" % (what, e, le))
    assert le <= 1e-5, (what, le)
    return W, loss


@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("dim", [4, 20, 64, 128])
def test_rows_and_losses_match_the_oracle(ctx, dim, epochs):
    wl, hist, w0 = make_case(10 + dim, SPAN + 17, dim, 19)
    check_against_oracle(ctx, wl, hist, w0, epochs, "dim %d epochs %d" % (dim, epochs))


@pytest.mark.parametrize("n_item", [1, 15, 16, 17, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3])
def test_item_tile_and_span_edges(ctx, n_item):
    wl, hist, w0 = make_case(300 + n_item, n_item, 20, 19)
    check_against_oracle(ctx, wl, hist, w0, 2, "n_item %d" % n_item)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 70])
def test_user_tile_edges(ctx, n):
    wl, hist, w0 = make_case(400 + n, SPAN + 17, 20, n)
    check_against_oracle(ctx, wl, hist, w0, 2, "n %d" % n)
    check_against_oracle(ctx, wl, hist, None, 2, "n %d from zeros" % n)


def test_a_users_bits_do_not_depend_on_the_call(ctx):
    wl, hist, w0 = make_case(77, 2 * SPAN + 3, 20, 70)
    me, mine = hist[5], w0[5:6]
    alone = raw_fold(ctx, wl, *csr([me]), 3, mine)
    again = raw_fold(ctx, wl, *csr([me]), 3, mine)
    np.testing.assert_array_equal(alone[0], again[0]); np.testing.assert_array_equal(alone[1], again[1])
    for pos in (0, 69):
        hh, ww = list(hist), w0.copy()
        hh[pos], ww[pos] = me, mine[0]
        a = raw_fold(ctx, wl, *csr(hh), 3, ww)
        b = raw_fold(ctx, wl, *csr(hh), 3, ww)
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])      # the identical call, twice
        np.testing.assert_array_equal(a[0][pos], alone[0][0]); np.testing.assert_array_equal(a[1][pos], alone[1][0])
    # among bad users: a target equal to n_item on one side, a negative id on the other
    n_item = wl.shape[0]
    hh = [np.array([3, n_item]), me, np.array([-1])]
    ctx.take_bad_ids()
    a = raw_fold(ctx, wl, *csr(hh), 3, np.concatenate([w0[:1], mine, w0[2:3]]))
    assert ctx.take_bad_ids() == 2
    np.testing.assert_array_equal(a[0][1], alone[0][0]); np.testing.assert_array_equal(a[1][1], alone[1][0])
    # in place (w_out aliases w0)
    a = raw_fold(ctx, wl, *csr([me]), 3, mine, in_place=True)
    np.testing.assert_array_equal(a[0], alone[0])


def test_logits_beyond_709_stay_finite(ctx):
    wl, hist, _ = make_case(88, SPAN + 17, 20, 19)
    w0 = f32(1000.0 * wl[np.arange(19) * 13 % wl.shape[0]])
    assert np.abs(wl @ w0.T).max() > 709
    W, loss = check_against_oracle(ctx, wl, hist, w0, 2, "w0 = 1000 wl[j]")
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(loss))


@pytest.mark.parametrize("dim", [20, 128])
def test_one_epoch_from_xu_is_the_xu_part_of_the_step(ctx, dim):
    ctx.set_batch_cap(1)
    alpha, lam = 0.01, 0.001
    pr = problem(500 + dim, SPAN + 17, dim, [1, 5, 12])
    for u in range(3):
        t, c = pr["data"][u]
        Q, _ = PO.step(pr["P"], pr["T"], u, t, c, float(np.float32(alpha)), float(np.float32(lam)), pr["len_max"])
        m = model_of(pr, alpha, lam)
        w = m.fold_in([t], epochs=1, init=pr["P"]["xu"][u:u + 1]).cpu().numpy()
        what = "dim %d user %d" % (dim, u)
        assert_close(w[0], Q["xu"][u], "fold-in vs oracle step " + what)
        assert_delta_close(w[0], Q["xu"][u], pr["P"]["xu"][u], "fold-in vs oracle step " + what)
        m.train(u)                                            # poi_poi2vec_step on a one-user launch at cap 1
        stepped = tables(m)["xu"][u]
        assert_close(stepped, Q["xu"][u], "step vs oracle step " + what)
        e = assert_close(w[0], stepped, "fold-in vs poi_poi2vec_step " + what, rtol=2 * RTOL)
        print(what, "fold-in vs step %.2e" % e)


def test_bad_input_and_nothing_to_do(ctx):
    wl, hist, w0 = make_case(99, 70, 20, 6)
    good = raw_fold(ctx, wl, *csr(hist), 2, w0)
    for r, bad in ((1, np.array([4, 70, 5])), (4, np.array([-3]))):
        hh = list(hist); hh[r] = bad
        ctx.take_bad_ids()
        W, loss = raw_fold(ctx, wl, *csr(hh), 2, w0)
        assert ctx.take_bad_ids() == 1
        assert np.all(np.isnan(W[r])) and np.all(np.isnan(loss[r]))
        keep = np.arange(6) != r
        np.testing.assert_array_equal(W[keep], good[0][keep]); np.testing.assert_array_equal(loss[keep], good[1][keep])
    off, flat = csr(hist)
    off2 = off.copy(); off2[3] = off[2] - 1                   # descending: users 2 and 3 read other ranges, user 2 has a negative length
    ctx.take_bad_ids()
    W, loss = raw_fold(ctx, wl, off2, flat, 2, w0)
    assert ctx.take_bad_ids() == 1 and np.all(np.isnan(W[2])) and np.all(np.isnan(loss[2]))
    keep = np.array([0, 1, 4, 5])
    np.testing.assert_array_equal(W[keep], good[0][keep]); np.testing.assert_array_equal(loss[keep], good[1][keep])
    # epochs = 0 and an empty history return w0 (zeros without it), losses 0
    W, loss = raw_fold(ctx, wl, off, flat, 0, w0)
    np.testing.assert_array_equal(W, w0.astype(np.float32)); assert loss.shape == (6, 0)
    hh = list(hist); hh[2] = np.zeros(0, np.int64)
    W, loss = raw_fold(ctx, wl, *csr(hh), 2, w0)
    np.testing.assert_array_equal(W[2], w0[2].astype(np.float32)); assert np.all(loss[2] == 0)
    np.testing.assert_array_equal(np.delete(W, 2, 0), np.delete(good[0], 2, 0))
    W, loss = raw_fold(ctx, wl, *csr(hh), 2, None)
    assert np.all(W[2] == 0) and np.all(loss[2] == 0)
    assert ctx.lib.poi_foldin_p2v(ctx.handle, None, 70, 20, None, None, 0, 2, 0.1, 0.0, None, None, None, None) != 0      # NULL wl
    torch.cuda.synchronize()


# ---- serving glue --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(ctx):
    pr = problem(600, 120, 20, [6, 3, 9, 1, 4])
    m = model_of(pr)
    rng = np.random.default_rng(8)
    hist = [rng.integers(0, 120, L) for L in (3, 1, 7, 12, 5, 2, 9)]
    kw = dict(epochs=4, alpha=ALPHA, lam=LAM, init="uniform", seed=3)
    W = m.fold_in(hist, **kw)
    # a second model whose trained xu rows ARE the folded rows, scored through the existing entries with the same contexts
    n = len(hist)
    pr2 = dict(pr, n_user=n, len_max=0, data={u: (np.zeros(0, np.int64), []) for u in range(n)},
               tes={u: (np.array([0]), [hist[u][-1:]]) for u in range(n)},
               P=dict(pr["P"], xu=W.cpu().numpy().astype(np.float64)))
    m2 = model_of(pr2, softmax_axis="items", eval_context="test")
    return pr, m, m2, hist, kw, W


def test_score_new_and_recommend_new_are_the_existing_entries_on_the_folded_rows(served):
    pr, m, m2, hist, kw, W = served
    users = np.arange(len(hist))
    full = m.score_new(hist, **kw)
    ref = m2.compute_sub_all_scores_device(users)
    assert full.shape == ref.shape == (len(hist), 120)
    assert torch.equal(full, ref)
    idx, sc = m.recommend_new(hist, 20, exclude=None, return_scores=True, **kw)
    ridx, rsc = m2.compute_sub_topk(users, 20, return_scores=True)
    assert torch.equal(idx, ridx) and torch.equal(sc, rsc)
    # the oracle on the folded rows: the glue scores what it says it scores
    got = full.cpu().numpy()
    for contexts in ("last", "none"):
        s = m.score_new(hist, contexts=contexts, **kw).cpu().numpy()
        assert_close(s, FO.scores(pr["P"], pr["T"], W.cpu().numpy(), hist, contexts), "score_new " + contexts)
    plu = PO.plu_matrix(dict(pr["P"], xu=W.cpu().numpy().astype(np.float64)), users, "items")
    assert_close(m.score_new(hist, contexts="none", **kw).cpu().numpy(), plu, "contexts='none' is plu alone")
    explicit = m.score_new(hist, contexts=[h[-1:] for h in hist], **kw)
    assert torch.equal(explicit, full)
    assert got.shape == (len(hist), 120)


def test_recommend_new_with_exclusion_lists(served):
    pr, m, m2, hist, kw, W = served
    got = m.score_new(hist, **kw).cpu().numpy()
    k = 10
    ro, rx = FO.history_exclusion(hist, 120)
    idx, sc, cnt = m.recommend_new(hist, k, return_scores=True, return_counts=True, **kw)
    ref, rc = FO.topk_ex(got, k, ro, rx)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rc)
    np.testing.assert_array_equal(sc.cpu().numpy(), np.take_along_axis(got, ref.astype(np.int64), 1))
    assert not np.any(np.isin(idx.cpu().numpy()[2], hist[2]))
    # a row with fewer than k candidates ends in -1 / NaN
    off = np.zeros(len(hist) + 1, np.int64)
    off[1:] = 117
    lists = (off, np.arange(3, 120))
    idx, sc, cnt = m.recommend_new(hist, k, exclude=lists, return_scores=True, return_counts=True, **kw)
    ref, rc = FO.topk_ex(got, k, off, np.arange(3, 120))
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    np.testing.assert_array_equal(idx, ref)
    assert np.all(rc == [3] + [120] * (len(hist) - 1)) and np.array_equal(cnt.cpu().numpy(), rc)
    assert np.all(idx[0, 3:] == -1) and np.all(np.isnan(sc[0, 3:])) and np.all(np.isfinite(sc[0, :3]))
    np.testing.assert_array_equal(sc[1:], np.take_along_axis(got, ref.astype(np.int64), 1)[1:])
    with pytest.raises(_lib.PoiError):
        m.recommend_new(hist, k, within_km=5.0, **kw)
    with pytest.raises(_lib.PoiError):
        m.rank_new(hist, np.zeros((len(hist), 1), np.int64), within_km=5.0, **kw)
    with pytest.raises(IndexError):
        m.fold_in([[1, 120]])                                 # the padding id is no POI of the softmax


def test_rank_new_and_foldin_rank_metrics(served):
    pr, m, m2, hist, kw, W = served
    got = m.score_new(hist, **kw).cpu().numpy()
    rng = np.random.default_rng(4)
    tgt = rng.integers(0, 120, (len(hist), 2))
    tgt[0, 0] = hist[0][0]                                    # an excluded target: not ranked
    tm = np.ones_like(tgt)
    ro, rx = FO.history_exclusion(hist, 120)
    for exclude, lists in (("history", (ro, rx)), (None, (None, None))):
        rank, cnt = m.rank_new(hist, (tgt, tm), exclude=exclude, return_counts=True, **kw)
        ref = RO.ranks(got, tgt, tm, *lists)
        np.testing.assert_array_equal(rank.cpu().numpy(), ref["rank"])
        np.testing.assert_array_equal(cnt.cpu().numpy(), ref["count"])
    assert ref["rank"].min() >= 0 and RO.ranks(got, tgt, tm, ro, rx)["rank"][0, 0] == -1
    fm = E.foldin_rank_metrics(m, hist, (tgt, tm), [1, 5, 120], **kw)
    assert set(fm) == {"n", "mrr", "mean_rank", "median_rank", "auc_full", "at"} and set(fm["at"]) == {1, 5, 120}
    s = RO.summary(RO.ranks(got, tgt, tm, ro, rx)["rank"], RO.ranks(got, tgt, tm, ro, rx)["count"])
    assert abs(fm["mrr"] - s["mrr"]) <= 1e-12 and abs(fm["mean_rank"] - s["mean_rank"]) <= 1e-9


def test_folded_rows_rank_held_out_check_ins_above_the_zero_row(ctx):
    """Strong generalisation: train on 320 users, fold the other 80 users' train check-ins in, rank their held-out next check-in.  The
    zero row (epochs = 0) scores by paths alone.  The inequality is first held on the CPU oracle, from the trained tables, so that it
    is the reference rule's own and not an accident of the kernel."""
    ctx.set_batch_cap(1)
    ds = D.make_poi2vec_synthetic(400, 600, 30, 13, local=0.5, n_nbr=8)
    p = dict(latent_size=20, seed=5, softmax_axis="items", eval_context="test")
    m = harness.poi2vec_model(ds, p)
    for epoch in range(4):
        order = np.random.default_rng(123 + epoch).permutation(320)
        for s in range(0, 320, 16):
            m.train_batch(order[s:s + 16], sync=False)
    m.ctx.take_bad_ids(m._stream().value)
    m.update_trained_params()
    off = ds.off.astype(np.int64)
    held = [u for u in range(320, 400) if off[u + 1] > off[u] and ds.tes_off[u + 1] > ds.tes_off[u]]
    hist = [ds.tra_t[off[u]:off[u + 1]].astype(np.int64) for u in held]
    tgt = np.array([[ds.tes_t[ds.tes_off[u]]] for u in held], np.int64)
    tm = np.ones_like(tgt)
    kw = dict(epochs=20, alpha=ALPHA, lam=LAM)
    # the oracle's own inequality
    P = dict(xu=np.zeros((1, 20)), wl=m._trained["wl"][:ds.n_item].cpu().numpy().astype(np.float64), pb=m._trained["pb"].cpu().numpy().astype(np.float64))
    T = dict(routes=ds.routes, lrs=ds.lrs, probs=ds.probs, n_node=ds.n_node)
    ro, rx = FO.history_exclusion(hist, ds.n_item)
    mrr = {}
    for name, ep in (("folded", 20), ("zero", 0)):
        W, _ = FO.fold_in(P["wl"], hist, ep, ALPHA, LAM)
        r = RO.ranks(FO.scores(P, T, W, hist, "last"), tgt, tm, ro, rx)
        mrr[name] = RO.summary(r["rank"], r["count"])["mrr"]
    fm = E.foldin_rank_metrics(m, hist, (tgt, tm), [5, 20], **kw)
    zm = E.foldin_rank_metrics(m, hist, (tgt, tm), [5, 20], **dict(kw, epochs=0))
    print("held-out users %d: oracle mrr folded %.4f zero %.4f; device mrr folded %.4f zero %.4f, recall@20 %.3f vs %.3f"
          % (len(held), mrr["folded"], mrr["zero"], fm["mrr"], zm["mrr"], fm["at"][20]["recall"], zm["at"][20]["recall"]))
    assert mrr["folded"] > mrr["zero"], mrr
    assert fm["mrr"] > zm["mrr"], (fm["mrr"], zm["mrr"])
    full = E.full_rank_metrics(m, harness.compute_start_end(ds.n_user, 400), [5, 20])
    assert set(fm) == set(full) and set(fm["at"][5]) == set(full["at"][5])
