"""-m gpu parity of the mini-batch `Lstm` / `Rnn` (public/GRU.py:502-657, :661-809; csrc/cells.hip) against the float64 oracle
tests/cells_oracle.py, itself held to autograd of the reference graph in tests/test_cells_cpu.py.  Bars: RTOL on the weights,
DELTA_RTOL per row on the update (tests/gpu_util.py), 2e-5 relative on the batch loss."""
import numpy as np
import pytest

from tests import cells_oracle as C
from tests.gpu_util import DELTA_RTOL, assert_close, assert_step_close, delta_excess, round_f32, toy_problem

pytestmark = pytest.mark.gpu

NAMES = ("lt", "ui", "wh", "bi")
CLASS = {"lstm": "Lstm", "rnn": "Rnn"}
KERNEL = {"lstm": 4, "rnn": 1}
ALPHA, LAM = 0.01, 0.001


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    poi_amd._lib.load()
    yield poi_amd
    poi_amd._lib.context(0).set_option("cell_grid", 0)


def _params(seed, T, cell):
    rng = np.random.default_rng(seed + 3000)
    P = C.init_params(rng, T["n_item"], T["dim"], cell)       # the reference's range: uniform(-0.5, 0.5)
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape)
    return round_f32(P)


def _model(pa, T, P, cell, **kw):
    return getattr(pa.models, CLASS[cell])(train=T["train"], test=T["test"], alpha_lambda=[ALPHA, LAM], n_user=T["n_user"],
                                           n_item=T["n_item"], n_in=T["dim"], n_hidden=T["dim"], init=P, **kw)


def _state(model):
    return {k: np.asarray(getattr(model, k).get_value(), np.float64) for k in NAMES}


def _snapshot(model):
    return [getattr(model, k).t.clone() for k in NAMES]


def _restore(model, snap):
    for k, t in zip(NAMES, snap):
        getattr(model, k).t.copy_(t)


def _bits(model):
    import torch
    torch.cuda.synchronize()
    return [getattr(model, k).t.view(torch.int32).clone() for k in NAMES]


def _check_step(model, P, T, idxs, cell, what):
    Pm, Qm, Mm = T["train"][0], T["train"][2], T["train"][1]
    exp, loss = C.minibatch_step(P, Pm[idxs], Qm[idxs], Mm[idxs], ALPHA, LAM, cell)
    got_loss = model.train(idxs)
    print("%s: loss %.9g oracle %.9g" % (what, got_loss, loss))
    assert_close(got_loss, loss, "batch loss " + what, rtol=2e-5)
    got = _state(model)
    worst = assert_step_close(got, exp, P, NAMES, what)
    print("%s: worst weight error %.3e" % (what, worst))
    return got, exp


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("dim,n_user,batch", [(20, 23, 7), (32, 40, 40), (64, 50, 16), (128, 40, 17), (256, 12, 12)])
def test_cell_steps_match_oracle(pa, cell, dim, n_user, batch):
    T = toy_problem(500 + dim, n_user=n_user, n_item=70, dim=dim, len_max=11, hot=8)
    P = _params(500 + dim, T, cell)
    model = _model(pa, T, P, cell)
    order = np.random.default_rng(2).permutation(n_user).astype(np.int32)
    for b0 in range(0, n_user, batch):                        # consecutive batches from the device state; the last one is ragged
        got, _ = _check_step(model, P, T, order[b0:b0 + batch], cell, "%s dim %d batch at %d" % (cell, dim, b0))
        P = dict(P, **got)
    assert model.ctx.last_plan("cell_kernel") == KERNEL[cell]
    assert model.ctx.last_plan("cell_grid") == min(batch, len(order[b0:]))


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_capped_grid_walks_the_batch_and_is_bitwise_equal(pa, cell):
    T = toy_problem(41, n_user=40, n_item=70, dim=32, len_max=11, hot=8)
    P = _params(41, T, cell)
    model = _model(pa, T, P, cell)
    idxs = np.random.default_rng(3).permutation(40).astype(np.int32)
    snap = _snapshot(model)
    l0 = model.train_batch(idxs)
    assert model.ctx.last_plan("cell_grid") == 40
    free = _bits(model)
    _restore(model, snap)
    model.ctx.set_option("cell_grid", 3)
    try:
        l1 = model.train_batch(idxs)
        assert model.ctx.last_plan("cell_grid") == 3 and model.ctx.last_plan("cell_kernel") == KERNEL[cell]
    finally:
        model.ctx.set_option("cell_grid", 0)
    import torch
    assert all(torch.equal(a, b) for a, b in zip(free, _bits(model)))
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    exp, _ = C.minibatch_step(P, T["train"][0][idxs], T["train"][2][idxs], T["train"][1][idxs], ALPHA, LAM, cell)
    assert_step_close(_state(model), exp, P, NAMES, "capped grid")


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_ill_conditioned_long_sequences_hold_both_bars(pa, cell):
    """dim 128, reference-range init, one user at the full 50 positions: where a float32 recurrence misses the contract."""
    T = toy_problem(9, n_user=8, n_item=70, dim=128, len_max=50, min_len=20, hot=8)
    assert T["lens"][0] == 50
    P = _params(9, T, cell)
    model = _model(pa, T, P, cell)
    _check_step(model, P, T, np.arange(8, dtype=np.int32), cell, "%s ill-conditioned" % cell)


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_hot_rows_cross_the_sort_windows(pa, cell):
    """64 users drawing every positive from 4 POIs: runs of several hundred entries per row, far beyond a 64-entry window."""
    T = toy_problem(17, n_user=64, n_item=40, dim=32, len_max=30, min_len=20, hot=4)
    P = _params(17, T, cell)
    model = _model(pa, T, P, cell)
    idxs = np.arange(64, dtype=np.int32)
    assert np.bincount(T["train"][0][T["train"][1] > 0], minlength=4)[:4].min() > 300
    got, exp = _check_step(model, P, T, idxs, cell, "%s hot rows" % cell)
    rows = [0, 1, 2, 3, T["n_item"]]                          # the hot rows and the pad row, on their own
    ex, _ = delta_excess(got["lt"][rows], exp["lt"][rows], P["lt"][rows], DELTA_RTOL)
    print("hot / pad rows: %.3f of the delta tolerance" % ex)
    assert ex <= 1.0
    assert np.any(exp["lt"][T["n_item"]] != P["lt"][T["n_item"]])


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_lengths_one_and_two_next_to_long_ones(pa, cell):
    T = toy_problem(23, n_user=6, n_item=50, dim=20, len_max=12, min_len=8, hot=8)
    Pm, Mm, Qm = T["train"]
    for u, L in ((1, 1), (3, 2)):
        Pm[u, L:] = T["n_item"]; Qm[u, L:] = T["n_item"]; Mm[u, L:] = 0
    P = _params(23, T, cell)
    model = _model(pa, T, P, cell)
    got, _ = _check_step(model, P, T, np.arange(6, dtype=np.int32), cell, "%s short and long" % cell)
    _check_step(model, dict(P, **got), T, np.array([1], np.int32), cell, "%s one user of length 1" % cell)


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_identical_launches_are_bitwise_identical(pa, cell):
    T = toy_problem(31, n_user=30, n_item=60, dim=64, len_max=11, hot=8)
    model = _model(pa, T, _params(31, T, cell), cell)
    idxs = np.random.default_rng(5).permutation(30).astype(np.int32)[:21]
    snap = _snapshot(model)
    runs = []
    import torch
    for _ in range(3):
        _restore(model, snap)
        loss = model.train_batch(idxs)
        runs.append((_bits(model), loss.view(np.uint32).copy()))
    for bits, loss in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], bits))
        assert np.array_equal(runs[0][1], loss)
    assert not torch.equal(runs[0][0][0], snap[0].view(torch.int32))


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("dim", [20, 128])
def test_predict_scores_and_topk(pa, cell, dim):
    T = toy_problem(700 + dim, n_user=70, n_item=90, dim=dim, len_max=11, hot=16)      # >= 64 users: handed over sorted by length, rows come back through out_row
    P = _params(700 + dim, T, cell)
    model = _model(pa, T, P, cell)
    model.update_trained_items()
    ids = np.random.default_rng(1).permutation(70).astype(np.int32)
    exp = C.predict(P, T["train"][0][ids], T["train"][1][ids], cell)
    got = model.predict(ids)
    print("predict %s dim %d: %.3e" % (cell, dim, assert_close(got, exp, "hts")))
    full = model.predict_device(np.arange(70, dtype=np.int32))
    assert np.array_equal(full.cpu().numpy()[ids], got)
    model.update_trained_users(full)
    sc = model.compute_sub_all_scores(np.arange(70, dtype=np.int32))
    ref = C.predict(P, T["train"][0], T["train"][1], cell) @ P["lt"][:T["n_item"]].T
    assert_close(sc, ref, "scores", rtol=1e-5)
    top = model.compute_sub_topk(np.arange(70, dtype=np.int32), 5).cpu().numpy()
    order = np.argsort(-sc, axis=1, kind="stable")[:, :5]
    assert np.array_equal(np.take_along_axis(sc, top.astype(np.int64), 1), np.take_along_axis(sc, order, 1))
    assert model.ctx.take_bad_ids() == 0


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_out_of_range_poi_raises_and_moves_nothing(pa, cell):
    T = toy_problem(3, n_user=9, n_item=40, dim=20, len_max=9, hot=8)
    model = _model(pa, T, _params(3, T, cell), cell)
    model.ctx.take_bad_ids()
    before = _bits(model)
    off = model._off_host
    good = model.q.clone()
    model.q[int(off[4]) + 1] = T["n_item"] + 7                 # past the pad row
    import torch
    with pytest.raises(IndexError):
        model.train(np.arange(9, dtype=np.int32))
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(model)))
    assert model.ctx.take_bad_ids() == 0                      # counted once, cleared by the raise
    loss = model.train_batch(np.array([0, 4, 2], np.int32), sync=False).cpu().numpy()
    assert np.isnan(loss[1]) and model.ctx.take_bad_ids() == 1
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(model)))
    model.q.copy_(good)
    assert np.isfinite(model.train(np.arange(9, dtype=np.int32)))
    with pytest.raises(ValueError):
        _model(pa, T, _params(3, T, cell), cell, table_dtype="f16")


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_train_minibatch_runs_epochs(pa, cell):
    p = pa.harness.minibatch_default_params()
    p.update(cell=cell, epochs=2, dataset="synthetic:tiny", latent_size=16, batch_size_train=8, alpha=0.1)
    model, best, hist = pa.harness.train_minibatch(None, p, log=lambda *a: None)
    assert type(model).__name__ == CLASS[cell] and len(hist) == 2
    losses = [h["loss"] for h in hist]
    print("%s epoch losses %s auc %s" % (cell, losses, [h["auc"] for h in hist]))
    assert all(np.isfinite(l) for l in losses) and losses[1] < losses[0]
    assert all(0.0 <= h["auc"] <= 1.0 and len(h["recall"]) == len(p["at_nums"]) for h in hist)
