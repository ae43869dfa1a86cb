"""-m gpu tests of the candidate generation (poi_score_rows, poi_topk_select, poi_score_candidates -> models.compute_sub_candidates,
Session.candidates, evaluate.candidate_recall).  The selection is held EXACTLY to the numpy oracle of tests/select_oracle.py on the
planted score rows of tests/select_cases.py - ids, scores and counts of every row; the score rows to the float64 oracle (near_oracle.scores) and bitwise
to poi_score_rank; the whole path to the ranks of compute_sub_target_rank, exactly; every grid, regime and chunking to the same bits."""
import ctypes

import numpy as np
import pytest

from tests import select_cases as SC
from tests import select_oracle as SO
from tests.gpu_util import RTOL
from tests.group_cases import N_ITEM, N_USER, NO_LAST, RANK_CASES, exclusion_lists, rank_case, wide_case
from tests.test_gpu_near import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa._lib.context(0)
    yield c
    for name, v in (("select_split_max", 256), ("select_grid", 0), ("select_chunk_mb", 1024)):
        c.set_option(name, v)


def dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def dev_ex(ex):
    """(off, ids) int32 device tensors; an empty id array still has an address."""
    return (None, None) if ex[0] is None else (dev(np.asarray(ex[0], np.int32)), dev(np.asarray(ex[1], np.int32) if len(ex[1]) else np.zeros(1, np.int32)))


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def topk_select(ctx, sc_dev, n_item, k, ex=(None, None)):
    """poi_topk_select on a device matrix (n, ld) -> (ids, scores, counts) numpy."""
    import torch
    n, ld = sc_dev.shape
    idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.poi_topk_select(ctx.handle, p(sc_dev), n, n_item, ld, k, p(ex[0]), p(ex[1]), p(idx), p(val), p(cnt), None))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_is_oracle(got, shape, with_lists, k, what):
    ids, val, cnt = SC.expected(shape, with_lists)
    w = min(k, ids.shape[1])
    assert got[0].shape == (ids.shape[0], k) and got[0].dtype == np.int32, what
    bad = np.nonzero((got[0][:, :w] != ids[:, :w]).any(axis=1))[0]
    assert len(bad) == 0, "%s: ids differ from the oracle's on rows %s (patterns %s)" % (what, bad[:8], [SC.pattern_of(r) for r in bad[:8]])
    assert same_bits(got[1][:, :w], val[:, :w]), "%s: scores differ from the oracle's" % what
    assert np.array_equal(got[2], cnt), "%s: counts" % what


# ---- 1: poi_topk_select against the oracle, every row of every fixture ------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_selection_is_the_oracle_on_every_row(ctx, shape):
    F = SC.fixture(shape)
    n, N = F["sc"].shape
    sc = dev(SC.padded(F["sc"]))
    ex = dev_ex(F["ex"])
    for k in SC.ks_of(N):
        for with_lists in (False, True):
            got = topk_select(ctx, sc, N, k, ex if with_lists else (None, None))
            assert_is_oracle(got, shape, with_lists, k, "%s k %d lists %s" % (shape, k, with_lists))
            assert ctx.last_plan("select_path") == (1 if n <= 256 else 0)
    assert ctx.take_bad_ids() == 0


@pytest.mark.parametrize("shape", ["odd", "big"])
def test_short_lists_are_bitwise_poi_topk(ctx, shape):
    """At k <= 64, on the rows without a -0.0 (poi_topk leaves its place unspecified): the bits of poi_topk."""
    import torch
    F = SC.fixture(shape)
    keep = [r for r in range(len(F["sc"])) if not np.any((F["sc"][r] == 0) & np.signbit(F["sc"][r]))]
    assert len(keep) >= 0.7 * len(F["sc"])
    sub = np.ascontiguousarray(F["sc"][keep])
    n, N = sub.shape
    sc = dev(sub)
    for k in (1, 20, 64):
        ti = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
        ts = torch.full((n, k), float("-inf"), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.poi_topk(ctx.handle, p(sc), n, N, k, p(ti), p(ts), None))
        got = topk_select(ctx, sc, N, k)
        assert np.array_equal(got[0], ti.cpu().numpy()), (shape, k)
        assert same_bits(got[1], ts.cpu().numpy()), (shape, k)


# ---- 2: grids, regimes ------------------------------------------------------------------------------------------------------------------
def test_every_grid_and_regime_gives_the_same_bits(ctx):
    """The plateau and straddling-tie rows in both regimes and for 1 / 2 / 7 / 64 slices; a row alone against the call of 300."""
    for shape in ("big", "many"):
        F = SC.fixture(shape)
        n, N = F["sc"].shape
        sc, ex = dev(SC.padded(F["sc"])), dev_ex(F["ex"])
        for k in (100, 1000):
            base = None
            for split_max, grid in ((0, 0), (1 << 30, 1), (1 << 30, 2), (1 << 30, 7), (1 << 30, 64), (1 << 30, 0)):
                ctx.set_option("select_split_max", split_max); ctx.set_option("select_grid", grid)
                got = topk_select(ctx, sc, N, k, ex)
                assert ctx.last_plan("select_path") == (1 if split_max else 0)
                assert grid == 0 or ctx.last_plan("select_splits") == grid
                assert_is_oracle(got, shape, True, k, "%s k %d split_max %d grid %d" % (shape, k, split_max, grid))
                if base is None:
                    base = got
                assert np.array_equal(got[0], base[0]) and same_bits(got[1], base[1]) and np.array_equal(got[2], base[2])
        ctx.set_option("select_split_max", 256); ctx.set_option("select_grid", 0)
    # a row alone (the split regime) against its place in the call of 300 (the row regime)
    F = SC.fixture("many")
    N = F["sc"].shape[1]
    whole = topk_select(ctx, dev(F["sc"]), N, 100)
    assert ctx.last_plan("select_path") == 0
    for r in (0, 1, 2, 5, 17, 299):
        alone = topk_select(ctx, dev(F["sc"][r:r + 1]), N, 100)
        assert ctx.last_plan("select_path") == 1
        assert np.array_equal(alone[0][0], whole[0][r]) and same_bits(alone[1][0], whole[1][r]) and alone[2][0] == whole[2][r], r


# ---- 3: contract of the entry ------------------------------------------------------------------------------------------------------------
def test_select_contract(ctx):
    import torch
    F = SC.fixture("odd")
    n, N = F["sc"].shape
    sc = dev(F["sc"])
    # malformed device lists: descending ids, an id outside the table, a repeated id - each row all -1, count 0, counted once
    lists = [[], [5, 3], [1, N], [2, 4, 4]] + [[7]] * (n - 4)
    off, ids = SO.csr(lists)
    got = topk_select(ctx, sc, N, 20, dev_ex((off, ids)))
    for r in (1, 2, 3):
        assert (got[0][r] == -1).all() and np.isneginf(got[1][r]).all() and got[2][r] == 0
    assert ctx.take_bad_ids() == 3
    want = SO.select(F["sc"], 20, off, ids)
    keep = [r for r in range(n) if r not in (1, 2, 3)]
    assert want[3] == 3 and np.array_equal(got[0][keep], want[0][keep]) and np.array_equal(got[2], want[2])
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    for k in (0, -1, N + 1, 4097):
        rc = ctx.lib.poi_topk_select(ctx.handle, p(sc), n, N, N, k, None, None, p(z), None, None, None)
        assert rc == -4, k                               # POI_ENOTSUP
    assert ctx.lib.poi_topk_select(ctx.handle, p(sc), n, N, N - 1, 5, None, None, p(z), None, None, None) == -1      # ld < n_item
    assert ctx.lib.poi_topk_select(ctx.handle, p(sc), 0, N, N, 5, None, None, p(z), None, None, None) == 0           # n = 0: a no-op
    assert (z == 0).all()


# ---- 4: poi_score_rows ---------------------------------------------------------------------------------------------------------------------
def model_rows(m, rows):
    """(users, items, term) as compute_sub_candidates hands them to the library."""
    ids, users, lo = m._users_rows(rows)
    items = m._items() if hasattr(m, "_items") else m.trained_items.t
    return users.contiguous(), items, m._rank_term(ids, lo)


def score_rows(pa, m, rows, extra=5):
    """poi_score_rows on the model's own rows into an (n, n_item + extra) buffer -> numpy (the pad columns must stay untouched)."""
    import torch
    users, items, term = model_rows(m, rows)
    n, ld = users.shape[0], m.n_item + extra
    out = torch.full((n, ld), 7.0, dtype=torch.float32, device=m.device)
    m.ctx.check(m.lib.poi_score_rows(m.ctx.handle, *m._tile_operands(users, items, m.kdim, term), pa.models._ptr(out), ld, m._stream()))
    got = out.cpu().numpy()
    assert (got[:, m.n_item:] == 7.0).all(), "poi_score_rows wrote beyond n_item"
    return got[:, :m.n_item]


def build_rank_model(pa, R):
    """The case's model; on the spatial case the rows of NO_LAST lose their last POI in the scoring snapshot."""
    m = R["C"]["build"](pa)
    if R["C"]["kind"] == "spatial":
        m._last_poi[list(NO_LAST)] = -1
    return m


def mask_of(n, N, ex):
    mask = np.ones((n, N), bool)
    if ex[0] is not None:
        for r in range(n):
            mask[r, ex[1][ex[0][r]:ex[0][r + 1]]] = False
    return mask


@pytest.mark.parametrize("kind,dim", RANK_CASES)
def test_score_rows_and_the_whole_path(pa, kind, dim):
    """poi_score_rows against the float64 oracle and bitwise poi_score_rank; the candidates of the whole path against the exact ranks
    of compute_sub_target_rank (both sides read the same score bits under one total order: no gap qualification) and, their first
    20, against the float64 oracle."""
    import torch
    R = rank_case(kind, dim)
    m = build_rank_model(pa, R)
    rows = np.arange(N_USER)
    has_last = np.ones(N_USER, bool)
    if kind == "spatial":
        has_last[list(NO_LAST)] = False                  # (poi_score_rank scores such a row from POI 0: not the same definition)
    got = score_rows(pa, m, rows)
    err = np.abs(got - R["sc"]).max()
    print("%s dim %d: max|score rows - oracle| = %.3g, bound %.3g" % (kind, dim, err, RTOL * np.abs(R["sc"]).max()))
    assert err <= RTOL * np.abs(R["sc"]).max()
    tg = np.random.default_rng(dim).integers(0, N_ITEM, (N_USER, 8))
    rank, s2 = m.compute_sub_target_rank(rows, targets=tg, return_scores=True)
    assert same_bits(s2.cpu().numpy()[has_last], np.take_along_axis(got, tg, 1)[has_last]), "the scores differ from poi_score_rank's"
    # the whole path: ids, scores, counts; first against poi_score_rows + the oracle of the selection, exactly
    for name, ex in (("", (None, None)), (", lists", exclusion_lists(dim, N_USER, N_ITEM))):      # (one list per user row)
        exd = None if ex[0] is None else dev_ex(ex)
        for k in (100, 1000):
            idx, sc, cnt = (t.cpu().numpy() for t in m.compute_sub_candidates(rows, k, exclude=exd, return_scores=True, return_counts=True))
            want = SO.select(got, k, ex[0], ex[1])
            assert np.array_equal(idx, want[0]) and same_bits(sc, want[1]) and np.array_equal(cnt, want[2]), (kind, dim, k, name)
        mask = mask_of(N_USER, N_ITEM, ex)
        check((torch.as_tensor(idx[:, :20].copy()), torch.as_tensor(sc[:, :20].copy()), torch.as_tensor(cnt)), R["sc"], mask, 20,
              "%s dim %d first 20%s" % (kind, dim, name))
        # the candidate set of a row == {j : rank(j) < k}, the list position of j == rank(j): every id of a few rows, 8 targets at a time
        for u in (0, 1, 17, 78):
            assert has_last[u]
            all_ids = np.arange(130 * 8).reshape(130, 8)
            tm = (all_ids < N_ITEM).astype(np.int32)
            rex = None
            if ex[0] is not None:
                lst = ex[1][ex[0][u]:ex[0][u + 1]]
                rex = dev_ex(SO.csr([lst] * 130))
            ranks = m.compute_sub_target_rank(np.full(130, u), targets=(np.minimum(all_ids, N_ITEM - 1), tm), exclude=rex).cpu().numpy().reshape(-1)[:N_ITEM]
            for k in (100, 1000):
                ids_k = idx[u, :k]                       # (idx holds k = 1000: a shorter list is its prefix, checked above against the oracle)
                live = ids_k[ids_k >= 0]
                assert set(live.tolist()) == set(np.nonzero((ranks >= 0) & (ranks < k))[0].tolist()), (kind, dim, u, k, name)
                assert np.array_equal(ranks[live], np.arange(len(live))), (kind, dim, u, k, name)
    assert m.ctx.take_bad_ids() == 0


def test_half_table(pa):
    from tests import diverse_cases as DC
    import torch
    H = DC.half_case()
    m = H["build"](pa)
    assert m.trained_items.t.dtype == torch.float16
    rows = np.arange(DC.N_USER)
    got = score_rows(pa, m, rows)
    assert np.abs(got - H["sc"]).max() <= RTOL * np.abs(H["sc"]).max()
    idx, sc, cnt = (t.cpu().numpy() for t in m.compute_sub_candidates(rows, 200, exclude=dev_ex(H["ex"]), return_scores=True, return_counts=True))
    want = SO.select(got, 200, *H["ex"])
    assert np.array_equal(idx, want[0]) and same_bits(sc, want[1]) and np.array_equal(cnt, want[2])
    check((torch.as_tensor(idx[:, :20].copy()), torch.as_tensor(sc[:, :20].copy()), torch.as_tensor(cnt)), H["sc"], mask_of(DC.N_USER, DC.N_ITEM, H["ex"]), 20,
          "half table first 20")


# ---- 5: chunks, regimes and grids of the whole path ---------------------------------------------------------------------------------------
def test_chunks_regimes_and_grids_give_the_same_bits(pa, ctx):
    """70 rows x 5000 POIs: "select_chunk_mb" = 1 holds one 32-row tile (640 KB) - three chunks; both regimes; 1 / 2 / 7 / 64 slices."""
    W = wide_case()
    m = W["C"]["build"](pa)
    assert m.ctx is ctx
    rows = np.arange(70)
    ex = dev_ex(SC.fixture("big")["ex"])                 # (70 lists over 5000 ids)
    run = lambda k: tuple(t.cpu().numpy() for t in m.compute_sub_candidates(rows, k, exclude=ex, return_scores=True, return_counts=True))
    for k in (100, 4096):
        base = run(k)
        assert ctx.last_plan("select_chunks") == 1 and ctx.last_plan("select_rows_per_chunk") == 96 and ctx.last_plan("select_path") == 1
        want = SO.select(score_rows(pa, m, rows), k, *SC.fixture("big")["ex"])
        assert np.array_equal(base[0], want[0]) and same_bits(base[1], want[1]) and np.array_equal(base[2], want[2])
        for chunk_mb, split_max, grid in ((1, 256, 0), (1, 0, 0), (1024, 0, 0), (1024, 256, 1), (1, 256, 2), (1024, 256, 7), (1, 256, 64)):
            ctx.set_option("select_chunk_mb", chunk_mb); ctx.set_option("select_split_max", split_max); ctx.set_option("select_grid", grid)
            got = run(k)
            assert ctx.last_plan("select_chunks") == (3 if chunk_mb == 1 else 1) and ctx.last_plan("select_rows_per_chunk") == (32 if chunk_mb == 1 else 96)
            assert ctx.last_plan("select_path") == (1 if split_max else 0) and (grid == 0 or ctx.last_plan("select_splits") == grid)
            assert np.array_equal(got[0], base[0]) and same_bits(got[1], base[1]) and np.array_equal(got[2], base[2]), (k, chunk_mb, split_max, grid)
        ctx.set_option("select_chunk_mb", 1024); ctx.set_option("select_split_max", 256); ctx.set_option("select_grid", 0)
    # a row alone against the call of 70
    for r in (0, 33, 69):
        one = tuple(t.cpu().numpy() for t in m.compute_sub_candidates(rows[r:r + 1], 4096, return_scores=True, return_counts=True))
        allr = tuple(t.cpu().numpy() for t in m.compute_sub_candidates(rows, 4096, return_scores=True, return_counts=True))
        assert np.array_equal(one[0][0], allr[0][r]) and same_bits(one[1][0], allr[1][r]) and one[2][0] == allr[2][r]


# ---- 6: evaluation ----------------------------------------------------------------------------------------------------------------------------
def test_candidate_recall_is_full_rank_metrics_recall(pa):
    from poi_amd import evaluate as E
    R = rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    se = [np.arange(0, 50), np.arange(50, N_USER)]
    ks = [1, 5, 20, 100, 1000]
    for exclude in ("train", None):
        got = E.candidate_recall(m, se, ks, exclude=exclude)
        want = E.full_rank_metrics(m, se, ks, exclude=exclude)
        print(exclude, got)
        assert want["n"] > 0 and got[1000] > got[1]
        for k in ks:
            assert got[k] == want["at"][k]["recall"], (exclude, k, got[k], want["at"][k]["recall"])
    with pytest.raises(ValueError):
        E.candidate_recall(m, se, [5, 5])


# ---- 7: sessions and the explicit-score path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "lstm"])
def test_session_candidates_is_the_model_path_on_the_same_states(pa, kind):
    import torch
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    if kind == "spatial":
        m = TS.spatial_model(pa, T, TS.spatial_init(32, T))
        s = m.session(n_slot=T["n_user"])
    else:
        m = TC.model(pa, "lstm", T, TC.params("lstm", 60, T))
        m.set_coords(T["coords"])
        s = m.cell_session(n_slot=T["n_user"])
    slots = np.arange(T["n_user"])
    for t in range(3):
        s.advance(slots[:-2], T["train"][0][:-2, t])     # the last two slots never check in: no distance term, h = 0 - a plateau
    lists = SO.csr([np.sort(np.random.default_rng(r).choice(300, r % 40, replace=False)) for r in range(T["n_user"])])
    got = s.candidates(slots, 100, exclude=dev_ex(lists), return_scores=True, return_counts=True)
    st = s.state()
    m.update_trained_users(torch.as_tensor(np.float32(st["h"])))
    if kind == "spatial":
        m.update_trained_sus(torch.as_tensor(st["sts"]))
        m._last_poi = dev(np.asarray(st["last_poi"], np.int32))
    want = m.compute_sub_candidates(slots, 100, exclude=dev_ex(lists), return_scores=True, return_counts=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    keep = [j for j in range(300) if j not in set(lists[1][lists[0][63]:lists[0][64]].tolist())]
    assert got[0][63].cpu().numpy().tolist() == keep[:100]              # the plateau of a fresh slot: the lowest ids that are not excluded
    # the list position of a candidate is its exact rank under the slot's state
    rank = s.rank_of(slots, got[0][:, :8].contiguous(), exclude=dev_ex(lists)).cpu().numpy()
    assert np.array_equal(rank, np.tile(np.arange(8), (T["n_user"], 1)))
    last = s.candidates(slots[:5], 299, exclude="last", return_counts=True)
    assert np.all(last[1].cpu().numpy() == T["n_item"] - 1) and not np.any(last[0].cpu().numpy() == st["last_poi"][:5, None])
    with pytest.raises(ValueError):
        s.candidates(slots, 100, exclude="train")
    with pytest.raises(ValueError):
        s.candidates(slots, 301)


def test_explicit_score_path_through_prme(pa):
    from poi_amd import data as D
    from tests.test_gpu_prme import _model
    ds = D.make_prme_synthetic(45, 700, 14, 4)
    m = _model(ds)
    m.update_trained_items()
    users = np.arange(ds.n_user)
    full = np.float32(m.compute_sub_all_scores(users).reshape(ds.n_user, -1, ds.n_item)[:, 0])       # row 0: the query is the last train POI
    lists = SO.csr([np.sort(np.random.default_rng(r).choice(ds.n_item, r % 50, replace=False)) for r in range(ds.n_user)])
    for k in (65, 140):
        idx, sc, cnt = (t.cpu().numpy() for t in m.compute_sub_candidates(users, k, exclude=dev_ex(lists), return_scores=True, return_counts=True))
        want = SO.select(full, k, *lists)
        assert np.array_equal(idx, want[0]) and same_bits(sc, want[1]) and np.array_equal(cnt, want[2]), k
    tr = m.compute_sub_candidates(users, 65, exclude="train", return_counts=True)
    eo, ei = (t.cpu().numpy() for t in m.train_exclusion())
    assert np.array_equal(tr[1].cpu().numpy(), ds.n_item - np.diff(eo))


def test_carnn_session_takes_the_explicit_score_path(pa):
    from tests.test_gpu_group import carnn_model
    m = carnn_model(pa)
    s = m.cell_session(n_slot=21)
    rng = np.random.default_rng(4)
    slots = np.arange(20)                                    # slot 20 never checks in
    for t in range(3):
        s.advance(slots, rng.integers(0, 150, 20))
    every = np.arange(21)
    pool_i, pool_s = s.recommend(every, 64, return_scores=True)
    idx, sc, cnt = s.candidates(every, 120, return_scores=True, return_counts=True)
    assert np.all(idx[20].cpu().numpy() == -1) and cnt[20] == 0 and np.all(cnt[:20].cpu().numpy() == 150)
    assert np.array_equal(idx[:20, :64].cpu().numpy(), pool_i[:20].cpu().numpy()) and same_bits(sc[:20, :64].cpu().numpy(), pool_s[:20].cpu().numpy())
    rank = s.rank_of(slots, idx[:20, 100:108].contiguous()).cpu().numpy()
    assert np.array_equal(rank, np.tile(np.arange(100, 108), (20, 1)))


# ---- 8: the contract of the Python surface -----------------------------------------------------------------------------------------------------
def test_python_contract(pa):
    R = rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    rows = np.arange(N_USER)
    eo, ei = exclusion_lists(20, N_USER, N_ITEM)
    clean = tuple(t.cpu().numpy() for t in m.compute_sub_candidates(rows, 100, exclude=dev_ex((eo, ei)), return_scores=True, return_counts=True))
    r_x = int(np.nonzero(np.diff(eo) >= 2)[0][0])
    e2 = ei.copy(); e2[eo[r_x]:eo[r_x] + 2] = e2[eo[r_x]:eo[r_x] + 2][::-1]
    with pytest.raises(IndexError):
        m.compute_sub_candidates(rows, 100, exclude=dev_ex((eo, e2)))
    got = tuple(t.cpu().numpy() for t in m.compute_sub_candidates(rows, 100, exclude=dev_ex((eo, e2)), return_scores=True, return_counts=True, sync=False))
    assert m.ctx.take_bad_ids() == 1
    assert np.all(got[0][r_x] == -1) and np.all(np.isneginf(got[1][r_x])) and got[2][r_x] == 0
    good = rows != r_x
    assert all(np.array_equal(x[good], y[good]) for x, y in zip(got, clean)), "the other rows changed"
    with pytest.raises((IndexError, ValueError)):
        m.compute_sub_candidates(rows, 100, exclude=(eo, e2))          # host lists are checked before the launch
    for k in (0, -3, 4097, N_ITEM + 1):
        with pytest.raises(ValueError):
            m.compute_sub_candidates(rows, k)
    with pytest.raises(ValueError):
        m.compute_sub_candidates(rows, 100, exclude="last")
    out = m.compute_sub_candidates(np.zeros(0, np.int64), 100, return_scores=True, return_counts=True)
    assert out[0].shape == (0, 100) and out[1].shape == (0, 100) and out[2].shape == (0,)
    assert m.ctx.take_bad_ids() == 0
    # compute_sub_topk(k > 64) stays loud: the short-list entries are unchanged
    with pytest.raises(pa._lib.PoiError):
        m.compute_sub_topk(rows, 65)
