"""-m gpu: the mini-batch Lstm / Rnn step and predict (csrc/cells.hip) against the float64 oracle at the launch sizes where the kernels
change what they do.  tests/test_gpu_cells.py stops at 64 users, 90 POIs and 30 positions: one sort pass, one block of the plan scan,
no second sequence for a workgroup, no capped grid, the smallest dense-gradient chunk.  The cases (tests/cells_cases.py, which mirrors
each switch as a pure function; tests/test_cells_cpu.py shows on the same data that a lost entry, an entry on the neighbouring row,
a pad multiplicity off by one and a silent user each break a bar held here):

  A  sort passes          n_item 510 | 511 (1 | 2 passes) and 262142 | 262143 (2 | 3): the sorted keys come back in the other buffer pair;
                          ragged (the pad row's analytic multiplicity) and full length (the sentinel in slot 2 P, the pad row must not move)
  B  plan blocks, grid    255 | 256 | 257, 513, 769 users: cell_plan_kernel's scan carries row offsets and the rejection count across
                          blocks of 256 (users of length 1 on both sides of the first boundary), the recurrent grid stops at 512 and walks
                          on; grids 3 and 512 bitwise equal; a rejected user in the second block moves nothing
  C  commit cap, chunks   2 P + 1 > 16384 entries (cell_commit's grid-stride loop); P far below the n x max_len bound the dense-gradient
                          chunks are sized for (most chunks empty); a chunk size that does not divide P
  D  window cap           5300 users of 50 positions: more than 8192 windows (cell_rows / cell_span loop), three sort passes
  E  dims                 4, 12, 100, 252: uneven contraction slices, ragged 64 x 64 tiles of cell_wgrad, NO = 1008 partial sums
  F  workspace reuse      513 users, 3, 513 others, 1 of length 1 on one context: nothing of a larger launch leaks into a smaller one
  G  predict              600 users, more than the grid

Every launch is held to the bars of tests/test_gpu_cells.py - RTOL on the tensors, DELTA_RTOL per row of the update, 2e-5 relative on
the batch loss - and, additionally, every lt row the oracle leaves alone must be bit-identical to its value before the launch.  Each
test asserts from the case's own counts that it crosses the switch it is named for.  Printed per launch: worst weight error, share of
the delta tolerance, the oracle's seconds and the launch's milliseconds (host clock around train())."""
import functools
import time

import numpy as np
import pytest

from tests import cells_cases as K
from tests import cells_oracle as C
from tests.gpu_util import DELTA_RTOL, assert_close, assert_step_close, delta_excess

pytestmark = pytest.mark.gpu

NAMES = ("lt", "ui", "wh", "bi")
CLASS = {"lstm": "Lstm", "rnn": "Rnn"}
KERNEL = {"lstm": 4, "rnn": 1}
ALPHA, LAM = 0.01, 0.001
LOOP_MAX_STEPS = 6000       # position rows up to which the per-sequence oracle (the definition) is used: 0.3 s of CPU at dim 8


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    poi_amd._lib.load()
    yield poi_amd
    poi_amd._lib.context(0).set_option("cell_grid", 0)


case_a, case_b, case_c1, case_c2, case_d, case_e = (functools.lru_cache(maxsize=None)(f) for f in
                                                    (K.case_a, K.case_b, K.case_c1, K.case_c2, K.case_d, K.case_e))


_params = functools.lru_cache(maxsize=4)(K.params)


def _model(pa, T, P, cell):
    return getattr(pa.models, CLASS[cell])(train=T["train"], test=T["test"], alpha_lambda=[ALPHA, LAM], n_user=T["n_user"],
                                           n_item=T["n_item"], n_in=T["dim"], n_hidden=T["dim"], init=P)


def _fresh(pa, T, cell, seed=1):
    P = _params(seed, T["n_item"], T["dim"], cell)
    return _model(pa, T, P, cell), P


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


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _oracle(P, T, idxs, cell):
    """The loop oracle (the definition) for launches it walks in about a second, the batched one (held to it at 1e-12) beyond."""
    pm, qm, mm = K.tables(T, idxs)
    t0 = time.perf_counter()
    step = C.minibatch_step if K.position_rows(T, idxs) <= LOOP_MAX_STEPS else C.minibatch_step_batched
    exp, loss = step(P, pm, qm, mm, ALPHA, LAM, cell)
    return exp, loss, C.touched_rows(pm, qm, T["n_item"] + 1), time.perf_counter() - t0


def _compare(got, got_loss, P, oracle, what, seconds=0.0):
    exp, loss, touched, t_or = oracle
    ex = max(delta_excess(got[k], exp[k], P[k], DELTA_RTOL)[0] for k in NAMES)
    moved = int((got["lt"][~touched] != P["lt"][~touched]).any(axis=1).sum())
    worst = max(float(np.max(np.abs(got[k] - exp[k])) / np.max(np.abs(exp[k]))) for k in NAMES)
    print("[cells] %-44s worst weight error %.3e | %.3f of the delta tolerance | loss %.9g oracle %.9g | untouched rows moved %d of %d | "
          "oracle %.2f s, launch %.2f ms" % (what, worst, ex, got_loss, loss, moved, int((~touched).sum()), t_or, 1e3 * seconds), flush=True)
    assert_close(got_loss, loss, "batch loss " + what, rtol=2e-5)
    assert_step_close(got, exp, P, NAMES, what)
    assert moved == 0, "%s: %d lt rows the oracle leaves untouched changed" % (what, moved)
    return got


def _check_step(model, P, T, idxs, cell, what):
    """One launch from the tables P (the device's own values) against the oracle -> the device tables after it."""
    oracle = _oracle(P, T, idxs, cell)
    t0 = time.perf_counter()
    got_loss = model.train(idxs)
    dt = time.perf_counter() - t0
    assert model.ctx.last_plan("cell_kernel") == KERNEL[cell] and model.ctx.last_plan("cell_grid") == K.rec_grid(len(idxs))
    return _compare(_state(model), got_loss, P, oracle, what, dt)


# ---- A: sort passes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("full", [False, True], ids=["ragged", "full"])
@pytest.mark.parametrize("n_item,passes", list(zip(K.A_N_ITEM, K.A_PASSES)))
def test_a_sort_passes(pa, cell, full, n_item, passes):
    T = case_a(n_item, full)
    idxs = np.arange(40, dtype=np.int32)
    assert K.sort_passes(n_item) == passes
    assert (K.pad_multiplicity(T, idxs) == 0) == full and T["len_max"] == 11
    assert K.windows(T, idxs) > 1
    model, P = _fresh(pa, T, cell)
    touched = C.touched_rows(*K.tables(T, idxs)[:2], n_item + 1)
    assert touched[n_item] == (not full) and touched[0] and touched[n_item - 1]
    _check_step(model, P, T, idxs, cell, "A %s n_item %d %s (%d passes)" % (cell, n_item, "full" if full else "ragged", passes))


# ---- B: plan blocks and the persistent grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("n", K.B_SIZES)
def test_b_plan_blocks_and_grid(pa, cell, n):
    T = case_b()
    idxs = K.b_users(T, n)
    lens = T["lens"][idxs]
    assert -(-n // K.PLAN_BLOCK) == {255: 1, 256: 1, 257: 2, 513: 3, 769: 4}[n]
    assert n <= 255 or lens[255] == 1
    assert n <= 256 or lens[256] == 1
    model, P = _fresh(pa, T, cell)
    _check_step(model, P, T, idxs, cell, "B %s n %d" % (cell, n))
    if n > K.GRID_MAX:
        assert model.ctx.last_plan("cell_grid") == 512


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_b_grid_3_and_512_are_bitwise_equal(pa, cell):
    T = case_b()
    idxs = K.b_users(T, 513)
    model, P = _fresh(pa, T, cell)
    snap = _snapshot(model)
    runs = []
    for grid in (0, 3, 0, 0):
        _restore(model, snap)
        model.ctx.set_option("cell_grid", grid)
        try:
            loss = model.train_batch(idxs)
            assert model.ctx.last_plan("cell_grid") == (grid or 512) and model.ctx.last_plan("cell_kernel") == KERNEL[cell]
        finally:
            model.ctx.set_option("cell_grid", 0)
        runs.append((_bits(model), loss.view(np.uint32).copy(), grid))
    for bits, loss, grid in runs[1:]:
        assert _same(runs[0][0], bits), "tables differ between grid 512 and a launch with cell_grid = %d" % grid
        assert np.array_equal(runs[0][1], loss), "losses differ between grid 512 and a launch with cell_grid = %d" % grid
    import torch
    assert not torch.equal(runs[0][0][0], snap[0].view(torch.int32))
    _compare(_state(model), float(np.sum(runs[0][1].view(np.float32), dtype=np.float64)), P, _oracle(P, T, idxs, cell), "B %s n 513 grids" % cell)


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_b_rejection_in_the_second_plan_block(pa, cell):
    """An out-of-range negative in the user at batch position 300 of 513: found by the workgroup that walks it, counted through cnt[3]
    next to the plan scan's own count - every write-back kernel of the launch returns."""
    import torch
    T = case_b()
    idxs = K.b_users(T, 513)
    model, P = _fresh(pa, T, cell)
    model.ctx.take_bad_ids()
    before = _bits(model)
    u = int(idxs[300])
    assert T["lens"][u] >= 2 and 300 >= K.PLAN_BLOCK
    good = model.q.clone()
    model.q[int(model._off_host[u]) + 1] = T["n_item"] + 7     # past the pad row
    with pytest.raises(IndexError):
        model.train(idxs)
    assert _same(before, _bits(model))
    assert model.ctx.take_bad_ids() == 0                      # counted once, cleared by the raise
    loss = model.train_batch(idxs, sync=False).cpu().numpy()
    assert np.flatnonzero(np.isnan(loss)).tolist() == [300] and model.ctx.take_bad_ids() == 1
    assert _same(before, _bits(model))
    model.q.copy_(good)
    _check_step(model, P, T, idxs, cell, "B %s n 513 after a rejected launch" % cell)
    assert model.ctx.take_bad_ids() == 0


# ---- C: commit cap and dense-gradient chunks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_c_commit_grid_cap(pa, cell):
    T = case_c1()
    idxs = np.arange(513, dtype=np.int32)
    assert T["len_max"] == 17 and T["lens"].min() >= 16 and K.sort_entries(T, idxs) > K.COMMIT_GRID_MAX
    model, P = _fresh(pa, T, cell)
    _check_step(model, P, T, idxs, cell, "C %s commit cap, %d entries" % (cell, K.sort_entries(T, idxs)))


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_c_most_dense_chunks_empty(pa, cell):
    T = case_c2()
    idxs = np.arange(64, dtype=np.int32)
    rows, ch = K.position_rows(T, idxs), K.chunk_rows(64, K.max_len(T))
    assert K.max_len(T) == 50 and T["lens"][idxs].max() == 2 and ch == 56
    assert K.DENSE_CHUNKS - -(-rows // ch) >= 60               # chunks whose first row lies past P: rA = rB = P
    model, P = _fresh(pa, T, cell)
    assert model.max_len == 50
    _check_step(model, P, T, idxs, cell, "C %s %d rows under a bound of %d" % (cell, rows, 64 * 50))


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_c_chunk_rows_not_dividing_the_position_rows(pa, cell):
    T = case_b()
    idxs = K.b_users(T, 257)
    rows, ch = K.position_rows(T, idxs), K.chunk_rows(257, K.max_len(T))
    assert ch == 48 and rows % ch != 0 and rows % 8 != 0 and rows < K.DENSE_CHUNKS * ch      # the last live chunk is cut at P, inside a group of 8 rows
    model, P = _fresh(pa, T, cell)
    _check_step(model, P, T, idxs, cell, "C %s %d rows in chunks of %d" % (cell, rows, ch))


# ---- D: window cap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_d_window_grid_cap(pa, cell):
    """The smallest launch past 8192 windows at this length (5200 users stay under it): the oracle is the batched one, the loop takes
    about half a minute here."""
    T = case_d()
    idxs = np.arange(K.D_N_USER, dtype=np.int32)
    assert K.position_rows(T, idxs) > 262144 and K.windows(T, idxs) > K.WINDOW_GRID_MAX and K.sort_passes(T["n_item"]) == 3
    assert K.sort_entries(T, idxs) > K.COMMIT_GRID_MAX and T["dim"] == 8
    mult = C.multiplicities(*K.tables(T, idxs)[:2], T["n_item"] + 1)
    assert mult[T["hot"]].min() > 40 * K.WINDOW and mult[T["n_item"]] == 3 and (mult == 1).sum() > 50_000      # rows with a single sorted entry
    model, P = _fresh(pa, T, cell, seed=90)
    _check_step(model, P, T, idxs, cell, "D %s n %d, %d windows" % (cell, len(idxs), K.windows(T, idxs)))


# ---- E: dims ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("dim", K.E_DIMS)
def test_e_dims(pa, cell, dim):
    T = case_e(dim)
    idxs = np.arange(9, dtype=np.int32)
    assert dim % 4 == 0 and dim % 16 != 0 and T["lens"].max() == 6
    model, P = _fresh(pa, T, cell)
    got = _check_step(model, P, T, idxs, cell, "E %s dim %d" % (cell, dim))
    model.update_trained_items()
    ids = np.random.default_rng(1).permutation(9).astype(np.int32)
    exp = C.predict(got, T["train"][0][ids], T["train"][1][ids], cell)
    print("[cells] E %s dim %d predict: %.3e" % (cell, dim, assert_close(model.predict(ids), exp, "hts")))
    assert model.ctx.take_bad_ids() == 0


# ---- F: workspace reuse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_f_smaller_launches_after_larger_ones(pa, cell):
    """513 users, 3, 513 others, one user of length 1, each from the tables the launch before left: window records, partial sums, sort
    buffers and plan tables of a larger launch stay in the workspace and must not reach a smaller one."""
    T = case_b()
    o = T["order"]
    model, P = _fresh(pa, T, cell)
    launches = [("513", o[:513]), ("3", o[600:603]), ("513 others", o[287:800]), ("1 of length 1", o[255:256])]
    assert T["lens"][o[255]] == 1 and len(np.intersect1d(o[:513], o[287:800])) < 513
    for what, idxs in launches:
        P = dict(P, **_check_step(model, P, T, idxs, cell, "F %s launch of %s" % (cell, what)))


# ---- G: predict beyond the grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "rnn"])
def test_g_predict_beyond_the_grid(pa, cell):
    T = case_b()
    model, P = _fresh(pa, T, cell)
    model.update_trained_items()
    model.ctx.take_bad_ids()
    ids = np.random.default_rng(8).permutation(K.B_N_USER)[:600].astype(np.int32)
    assert len(ids) > K.GRID_MAX and not np.all(np.diff(ids) == 1)
    exp = C.predict_batched(P, T["train"][0], T["train"][1], cell)
    got = model.predict(ids)
    print("[cells] G %s predict of 600 permuted users: %.3e" % (cell, assert_close(got, exp[ids], "hts, permuted ids")))
    full = model.predict_device(np.arange(600, dtype=np.int32)).cpu().numpy()
    print("[cells] G %s predict_device of users 0 .. 599: %.3e" % (cell, assert_close(full, exp[:600], "hts, predict_device")))
    both = ids < 600
    assert np.array_equal(full[ids[both]], got[both])
    assert model.ctx.take_bad_ids() == 0
