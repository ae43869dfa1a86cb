"""-m gpu: the serving paths that build explicit score rows a bounded number at a time (models._Base._row_chunks and the drivers that
iterate it) must not depend on where the rows are cut.  Every path is run twice on N = 7 rows - in one piece, and with the instance's
SCORE_ROWS_BYTES lowered so that the rows come in chunks of 3, 3 and 1 - and the two results must be the same bits (int views, so a NaN
must sit in the same place).  The uncut results are what the other test modules pin to the float64 oracles at these shapes.
The exclusion lists are laid out against the cuts: list 0 is empty, the last list is not, and the lists on both sides of either cut
(rows 2 | 3 and 5 | 6) are non-empty, so a chunk that took its window of the offsets one row off would read another row's ids."""
from contextlib import contextmanager

import numpy as np
import pytest

from tests.test_gpu_session import geo_problem, spatial_init, spatial_model

pytestmark = pytest.mark.gpu

N, STEP = 7, 3
CUTS = [(0, 3), (3, 3), (6, 1)]
EX_LEN = (0, 2, 3, 2, 0, 4, 1)
ALL = dict(return_scores=True, return_counts=True)


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def flat(out):
    """A result (a tensor, or a tuple that may hold the pool pair) -> the list of its arrays as int views."""
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in flat(o)]
    a = out.cpu().numpy()
    return [a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a]


@contextmanager
def budget(m, rows):
    m.SCORE_ROWS_BYTES = 4 * m.n_item * rows
    try:
        yield
    finally:
        del m.SCORE_ROWS_BYTES


def cut_and_uncut(m, call, what, cuts=CUTS):
    """call() in one piece and in chunks -> the uncut result, after asserting that the two are the same bits."""
    assert list(m._row_chunks(N)) == [(0, N)], "%s: the uncut call is cut" % what
    want = call()
    with budget(m, STEP):
        assert list(m._row_chunks(N)) == cuts, "%s: the rows are not cut as the test means them to be" % what
        got = call()
    a, b = flat(got), flat(want)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), "%s: output %d differs between the cut and the uncut call" % (what, i)
    return want


def exclusion(seed, n_item, lens=EX_LEN):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    return off, np.concatenate([np.sort(rng.choice(n_item, l, replace=False)) for l in lens]).astype(np.int32)


def targets(seed, n_item):
    rng = np.random.default_rng(seed)
    tgt = np.stack([rng.choice(n_item, 2, replace=False) for _ in range(N)]).astype(np.int32)
    tm = np.ones_like(tgt)
    tm[2, 1] = 0
    return tgt, tm


def masks(seed, n_item):
    rng = np.random.default_rng(seed)
    return rng.random((3, n_item)) < np.array([0.6, 0.3, 0.9])[:, None]


WHICH = np.array([0, 1, 2, 2, 1, 0, 1])


# ---- the models (n_user 24, n_item about 50, dim 8) --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def carnn(pa):
    from tests.test_gpu_session_cells import model, params
    T = geo_problem(71, n_user=24, n_item=50, n_dist=11, dim=8, len_min=4, len_max=8)
    m = model(pa, "carnn", T, params("carnn", 71, T))
    m.update_trained_users(m.predict_device(np.arange(24)))
    return T, m


@pytest.fixture(scope="module")
def prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(24, 50, 10, 4)
    m = _model(ds, dim=8)
    m.update_trained_items()
    m.set_coords(np.asarray(ds.coords, np.float64)[:ds.n_item])
    return ds, m


@pytest.fixture(scope="module")
def poi2vec(pa):
    """Users with 1 .. 3 test positions, so that the score rows are (user, position) rows: of USERS the first two chunks hold a user with
    three positions and the last chunk's user has two."""
    from tests.test_gpu_poi2vec import model_of, problem
    rng = np.random.default_rng(19)
    pr = problem(300, 50, 8, [int(x) for x in rng.integers(3, 9, 24)])
    for u in range(24):
        k = 1 + (u // 2) % 3
        pr["tes"][u] = (rng.integers(0, 50, k), [rng.integers(0, 50, rng.integers(1, 4)) for _ in range(k)])
    m = model_of(pr, softmax_axis="items", eval_context="test")
    m.update_trained_params()
    return pr, m


USERS = np.array([3, 4, 5, 9, 11, 12, 20])


def histories(seed, n_item):
    rng = np.random.default_rng(seed)
    return [list(rng.integers(0, n_item, rng.integers(2, 7))) for _ in range(N)]


# ---- the models' own score rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["carnn", "prme"])
def test_model_side_paths(pa, request, kind):
    m = request.getfixturevalue(kind)[1]
    ex = exclusion(1, m.n_item)
    filt = pa.models.PoiFilter.from_masks(m, masks(2, m.n_item))
    geo_weight = 0.5 if kind == "carnn" else 1.0              # PRME has no single POI table for the embedding similarity
    rank, sc, cnt = cut_and_uncut(m, lambda: m.compute_sub_target_rank(USERS, exclude=ex, targets=targets(3, m.n_item), **ALL), kind + " rank")
    assert (rank.cpu().numpy() >= 0).sum() >= N
    idx = cut_and_uncut(m, lambda: m.compute_sub_candidates(USERS, 10, exclude=ex, **ALL), kind + " candidates")[0]
    assert (idx.cpu().numpy() >= 0).all()
    cut_and_uncut(m, lambda: m.compute_sub_topk_filtered(USERS, 5, filt, which=WHICH, exclude=ex, **ALL), kind + " filtered")
    cut_and_uncut(m, lambda: m.compute_sub_topk_diverse(USERS, 5, pool=16, trade=0.6, geo_weight=geo_weight, exclude=ex, return_objective=True,
                                                        return_pool=True, **ALL), kind + " diverse")
    cut_and_uncut(m, lambda: m.compute_sub_topk(USERS, 40, return_scores=True), kind + " top-40")


def test_poi2vec_user_position_rows(poi2vec):
    """(user, position) rows: the branch of the rank driver that hands every position of a user the user's exclusion list."""
    pr, m = poi2vec
    assert m.tes_masks.cpu().numpy()[USERS].sum(1).tolist() == [2, 3, 3, 2, 3, 1, 2]
    rank, sc, cnt = cut_and_uncut(m, lambda: m.compute_sub_target_rank(USERS, exclude=exclusion(4, m.n_item), **ALL), "poi2vec rank")
    assert (rank.cpu().numpy()[:, 1:] >= 0).any() and (rank.cpu().numpy()[6, 2] == -1)
    m.softmax_axis = "reference"                             # a softmax over the USERS of a call: such a call is never cut
    try:
        with budget(m, STEP):
            assert list(m._row_chunks(N)) == [(0, N)]
    finally:
        m.softmax_axis = "items"


# ---- fold-in: rank_new -------------------------------------------------------------------------------------------------------------------
def test_rank_new_prme(prme):
    ds, m = prme
    hist = histories(5, m.n_item)
    gaps = [list(np.random.default_rng(6 + i).integers(1, 700, len(h))) for i, h in enumerate(hist)]
    rank = cut_and_uncut(m, lambda: m.rank_new(hist, gaps, targets(7, m.n_item), exclude=exclusion(8, m.n_item), epochs=2, **ALL), "prme rank_new")[0]
    assert (rank.cpu().numpy() >= 0).any()
    cut_and_uncut(m, lambda: m.rank_new(hist, gaps, targets(7, m.n_item), epochs=2, **ALL), "prme rank_new, exclude='history'")


def test_rank_new_geoie(pa):
    from poi_amd import data as D
    from tests.test_gpu_geoie import _model
    ds = D.make_synthetic(24, 50, 10, 5)
    m = _model(ds, dim=8, d_min=0.01)
    m.train_batch(np.arange(ds.n_user))
    m.update_trained()
    hist = histories(9, m.n_item)
    rank = cut_and_uncut(m, lambda: m.rank_new(hist, targets(10, m.n_item), exclude=exclusion(11, m.n_item), **ALL), "geoie rank_new")[0]
    assert (rank.cpu().numpy() >= 0).any()
    cut_and_uncut(m, lambda: m.rank_new(hist, targets(10, m.n_item), **ALL), "geoie rank_new, exclude='history'")


def test_rank_new_poi2vec(poi2vec):
    pr, m = poi2vec
    hist = histories(12, m.n_item)
    rank = cut_and_uncut(m, lambda: m.rank_new(hist, targets(13, m.n_item), exclude=exclusion(14, m.n_item), epochs=2, **ALL), "poi2vec rank_new")[0]
    assert (rank.cpu().numpy() >= 0).any()
    m.softmax_axis = "reference"                             # the folded rows are scored over the POIs whatever the model's axis: still cut
    try:
        with budget(m, STEP):
            assert m._rank_chunk(N) == N
            cut = m.rank_new(hist, targets(13, m.n_item), exclude=exclusion(14, m.n_item), epochs=2)
    finally:
        m.softmax_axis = "items"
    assert np.array_equal(cut.cpu().numpy(), rank.cpu().numpy())


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------
def test_carnn_cell_session(pa, carnn):
    """A slot without a check-in (no last POI: -1 ids, rank -1, NaN score, count 0) sits in the middle chunk."""
    import torch
    T, m = carnn
    s = m.cell_session(n_slot=25)
    s.replay(T["off"], T["p_flat"])
    slots = np.array([0, 1, 2, 3, 24, 5, 6])
    ex = exclusion(15, m.n_item)
    filt = pa.models.PoiFilter.from_masks(m, masks(16, m.n_item))
    rank, sc, cnt = cut_and_uncut(m, lambda: s.rank_of(slots, targets(17, m.n_item)[0], exclude=ex, **ALL), "session rank_of")
    assert (rank[4] == -1).all() and torch.isnan(sc[4]).all() and cnt[4] == 0 and (rank.cpu().numpy() >= 0).sum() >= N
    idx, sc, cnt = cut_and_uncut(m, lambda: s.candidates(slots, 10, exclude=ex, **ALL), "session candidates")
    assert (idx[4] == -1).all() and cnt[4] == 0 and (idx.cpu().numpy()[[0, 1, 2, 3, 5, 6]] >= 0).all()
    idx, sc, cnt = cut_and_uncut(m, lambda: s.recommend_filtered(slots, 5, filt, which=WHICH, exclude=ex, **ALL), "session filtered")
    assert (idx[4] == -1).all() and cnt[4] == 0
    out = cut_and_uncut(m, lambda: s.recommend_diverse(slots, 5, pool=16, trade=0.6, geo_weight=0.5, exclude=ex, return_objective=True,
                                                       return_pool=True, **ALL), "session diverse")
    assert (out[0][4] == -1).all() and out[-1][4] == 0
    idx, sc = cut_and_uncut(m, lambda: s.recommend(slots, 40, return_scores=True), "session recommend")
    assert (idx[4] == -1).all() and torch.isnan(sc[4]).all() and (idx.cpu().numpy()[[0, 1, 2, 3, 5, 6]] >= 0).all()


def test_spatial_session_recommend_beyond_the_fused_k(pa):
    T = geo_problem(72, n_user=24, n_item=50, n_dist=11, dim=8, len_min=4, len_max=8)
    m = spatial_model(pa, T, spatial_init(72, T))
    s = m.session(n_slot=25)
    s.replay(T["off"], T["p_flat"])
    idx, sc = cut_and_uncut(m, lambda: s.recommend(np.array([0, 1, 2, 3, 24, 5, 6]), 40, return_scores=True), "spatial session top-40")
    assert (idx.cpu().numpy() >= 0).all()


def test_groups_come_whole_within_the_row_budget(carnn):
    """Three groups of two members under a budget of four rows: two launches, of four rows and of two."""
    T, m = carnn
    groups = [[3, 9], [4, 11], [12, 20]]
    ex = exclusion(18, m.n_item, (0, 3, 2))
    want = m.recommend_group(groups, 5, agg="min", exclude=ex, **ALL)
    launches, rows_of = [], m._rank_score_rows
    m._rank_score_rows = lambda a: (launches.append(len(a)), rows_of(a))[1]
    try:
        with budget(m, 4):
            got = m.recommend_group(groups, 5, agg="min", exclude=ex, **ALL)
    finally:
        del m._rank_score_rows
    assert launches == [4, 2]
    assert all(np.array_equal(x, y) for x, y in zip(flat(got), flat(want))) and (want[0].cpu().numpy() >= 0).all()
