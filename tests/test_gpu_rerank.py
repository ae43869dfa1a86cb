"""-m gpu tests of the re-ranking (poi_score_lists, poi_rerank_lists, poi_rerank -> models.score_lists / rerank, Session.rerank,
evaluate.two_stage_metrics).  poi_rerank_lists is held EXACTLY to the numpy oracle of tests/rerank_oracle.py on the planted lists of
tests/rerank_cases.py - ids, key bits, positions and counts of every row; poi_score_lists bitwise to the listed columns of
poi_score_rows and within RTOL of the float64 oracle; the fused entry to the two calls; every layout and grid to the same bits."""
import numpy as np
import pytest

from tests import rerank_cases as RC
from tests import rerank_oracle as RO
from tests.gpu_util import RTOL
from tests.group_cases import N_ITEM, N_USER, RANK_CASES, rank_case, tiny_case
from tests.test_gpu_select import build_rank_model, dev, model_rows, p, same_bits, score_rows

pytestmark = pytest.mark.gpu
ENOTSUP = -4


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    assert poi_amd._lib.load().poi_score_lists_chunk() == RC.CHUNK
    return poi_amd


@pytest.fixture(scope="module")
def ctx(pa):
    return pa._lib.context(0)


def dev_ids(a):
    """int32 device tensor; an empty array still has an address."""
    a = np.asarray(a, np.int32)
    return dev(a if a.size else np.zeros(1, np.int32))


def dev_f(a):
    a = np.asarray(a, np.float32)
    return dev(a if a.size else np.zeros(1, np.float32))


def rerank_lists(ctx, off, cand, n, score, k, prior=None, weights=RC.WEIGHTS, rc_want=0):
    """poi_rerank_lists -> (ids, keys, positions, counts) numpy."""
    import torch
    idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    pos = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    o, c, s, pr = None if off is None else dev_ids(off), dev_ids(cand), dev_f(score), None if prior is None else dev_f(prior)      # (alive over the call)
    rc = ctx.lib.poi_rerank_lists(ctx.handle, p(o), p(c), n, len(cand), p(s), p(pr), weights[0], weights[1], k, p(idx), p(val), p(pos), p(cnt), None)
    assert rc == rc_want, (rc, rc_want)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), pos.cpu().numpy(), cnt.cpu().numpy()


# ---- 1: poi_rerank_lists against the oracle, every row of every fixture --------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(RC.SHAPES) + list(RC.SHARED))
def test_rerank_lists_is_the_oracle_on_every_row(ctx, shape):
    F = RC.any_fixture(shape)
    for with_prior in (False, True):
        ids, val, pos, cnt, bad = RC.expected(shape, with_prior)
        assert bad == F["bad"]
        for k in RC.KS:
            got = rerank_lists(ctx, F["off"], F["cand"], F["n"], F["score"], k, F["prior"] if with_prior else None)
            what = "%s k %d prior %s" % (shape, k, with_prior)
            wrong = np.nonzero((got[0] != ids[:, :k]).any(axis=1))[0]
            assert len(wrong) == 0, "%s: ids differ from the oracle's on rows %s (lengths %s)" % (what, wrong[:8], RC.lengths(F)[wrong[:8]])
            assert same_bits(got[1], val[:, :k]), "%s: keys differ from the oracle's" % what
            assert np.array_equal(got[2], pos[:, :k]), "%s: positions" % what
            assert np.array_equal(got[3], cnt), "%s: counts" % what
            assert ctx.take_bad_ids() == F["bad"], what


# ---- 2: poi_score_lists against poi_score_rows and the float64 oracle -------------------------------------------------------------------------
def score_lists(pa, m, rows, off, cand):
    """poi_score_lists on the model's own rows -> numpy scores (flat for ragged lists, (n, C) for a shared one); guard cells untouched."""
    import torch
    users, items, term = model_rows(m, rows)
    n = users.shape[0]
    numel = len(cand) if off is not None else n * len(cand)
    out = torch.full((numel + 5,), 7.0, dtype=torch.float32, device=m.device)
    o, c = None if off is None else dev_ids(off), dev_ids(cand)
    m.ctx.check(m.lib.poi_score_lists(m.ctx.handle, *m._tile_operands(users, items, m.kdim, term), p(o), p(c), len(cand),
                                      pa.models._ptr(out), m._stream()))
    got = out.cpu().numpy()
    assert (got[numel:] == 7.0).all(), "poi_score_lists wrote beyond its output"
    assert m.ctx.last_plan("lists_path") == (0 if off is not None else 1)
    return got[:numel] if off is not None else got[:numel].reshape(n, len(cand))


def check_against_rows(pa, m, full, oracle_sc, seed, what):
    """Ragged and shared lists with duplicates and padding: the bits of poi_score_rows' listed columns; the float64 oracle within RTOL."""
    n, N = full.shape
    rows = np.arange(n)
    off, cand = RC.scoring_lists(n, N, seed)
    got = score_lists(pa, m, rows, off, cand)
    want, bad = RO.score_lists(full, off, cand)
    assert bad == 0 and same_bits(got, want), "%s: ragged scores differ from poi_score_rows'" % what
    shared = RC.id_list(RC.CHUNK + 33, N, np.random.default_rng(seed), 1)[0]
    got_s = score_lists(pa, m, rows, None, shared)
    want_s, bad = RO.score_lists(full, None, shared)
    assert bad == 0 and same_bits(got_s, want_s), "%s: shared scores differ from poi_score_rows'" % what
    if oracle_sc is not None:
        oracle_sc = oracle_sc[:, :N]
        live = shared >= 0
        err = np.abs(got_s[:, live] - oracle_sc[:, shared[live]]).max()
        bound = RTOL * np.abs(oracle_sc).max()
        print("%s: max|score lists - float64 oracle| = %.3g, bound %.3g" % (what, err, bound))
        assert err <= bound
    assert m.ctx.take_bad_ids() == 0
    return off, cand, got


@pytest.mark.parametrize("kind,dim", RANK_CASES)
def test_score_lists_has_the_bits_of_score_rows(pa, kind, dim):
    R = rank_case(kind, dim)
    m = build_rank_model(pa, R)
    full = score_rows(pa, m, np.arange(N_USER), extra=0)
    check_against_rows(pa, m, full, R["sc"], dim, "%s dim %d" % (kind, dim))


def test_score_lists_on_a_half_table(pa):
    import torch
    from tests import diverse_cases as DC
    H = DC.half_case()
    m = H["build"](pa)
    assert m.trained_items.t.dtype == torch.float16
    full = score_rows(pa, m, np.arange(DC.N_USER), extra=0)
    check_against_rows(pa, m, full, H["sc"], 5, "half table")


@pytest.mark.parametrize("n_item", [13, 5])
def test_score_lists_on_tiny_tables(pa, n_item):
    Y = tiny_case(n_item)
    T = Y["T"]
    m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=n_item, n_in=8, n_hidden=8,
                         init=dict(ux=Y["users"], lt=Y["items"]))
    m.update_trained_items(); m.update_trained_users()
    full = score_rows(pa, m, np.arange(T["n_user"]), extra=0)
    check_against_rows(pa, m, full, Y["sc"], n_item, "tiny %d" % n_item)


# ---- 3: layouts and grids -----------------------------------------------------------------------------------------------------------------------
def test_layouts_and_call_sizes_give_the_same_bits(pa):
    """Ragged lists that all hold the same ids against the shared layout; a row alone against its place in a call of 300."""
    R = rank_case("spatial", 128)
    m = build_rank_model(pa, R)
    rows = np.arange(N_USER)
    shared = RC.id_list(RC.CHUNK + 1, N_ITEM, np.random.default_rng(8), 1)[0]
    one = score_lists(pa, m, rows, None, shared)
    off, cand = RO.csr([shared] * N_USER)
    assert same_bits(score_lists(pa, m, rows, off, cand).reshape(N_USER, -1), one)
    many = np.arange(300) % N_USER
    off, cand = RC.scoring_lists(300, N_ITEM, 9)
    whole = score_lists(pa, m, many, off, cand)
    for r in (0, 1, 77, 131, 299):
        alone = score_lists(pa, m, many[r:r + 1], np.array([0, off[r + 1] - off[r]]), cand[off[r]:off[r + 1]])
        assert same_bits(alone, whole[off[r]:off[r + 1]]), r
    assert m.ctx.take_bad_ids() == 0


# ---- 4: the fused entry is the two calls --------------------------------------------------------------------------------------------------------
def fused(pa, m, rows, off, cand, k, prior=None, weights=RC.WEIGHTS):
    import torch
    users, items, term = model_rows(m, rows)
    n = users.shape[0]
    idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    pos = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    o, c, pr = None if off is None else dev_ids(off), dev_ids(cand), None if prior is None else dev_f(prior)
    m.ctx.check(m.lib.poi_rerank(m.ctx.handle, *m._tile_operands(users, items, m.kdim, term), p(o), p(c), len(cand),
                                 p(pr), weights[0], weights[1], k, p(idx), p(val), p(pos), p(cnt), m._stream()))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), pos.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128), ("fpmc", 128)])
def test_fused_is_score_lists_then_rerank_lists(pa, ctx, kind, dim):
    R = rank_case(kind, dim)
    m = build_rank_model(pa, R)
    rows = np.arange(N_USER)
    rng = np.random.default_rng(dim)
    for off, cand in (RC.scoring_lists(N_USER, N_ITEM, dim), (None, RC.id_list(RC.CHUNK + 33, N_ITEM, rng, 1)[0])):
        sc = score_lists(pa, m, rows, off, cand)
        prior = rng.integers(-2, 3, sc.shape).astype(np.float32)
        for k in (20, 1025):
            for pr in (None, prior):
                two = rerank_lists(ctx, off, cand, N_USER, sc, k, pr)
                got = fused(pa, m, rows, off, cand, k, pr)
                assert np.array_equal(got[0], two[0]) and same_bits(got[1], two[1]) and np.array_equal(got[2], two[2]) and np.array_equal(got[3], two[3])
                want = RO.rerank(off, cand, N_USER, sc, k, pr, RC.WEIGHTS)
                assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[3], want[3])
    assert ctx.take_bad_ids() == 0


# ---- 5: a model's second stage applied to its own first stage changes nothing ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 20), ("spatial", 128)])
def test_reranking_the_models_own_candidates_changes_nothing(pa, kind, dim):
    R = rank_case(kind, dim)
    m = build_rank_model(pa, R)
    rows = np.arange(N_USER)
    idx, sc = (t.cpu().numpy() for t in m.compute_sub_candidates(rows, 100, return_scores=True))
    off, cand = RO.csr_of_padded(idx)
    got = fused(pa, m, rows, off, cand, 100)
    assert np.array_equal(got[0], idx) and same_bits(got[1], sc + np.float32(0.0))
    assert np.array_equal(got[2], np.tile(np.arange(100), (N_USER, 1))) and np.all(got[3] == 100)


# ---- 6: rejections -----------------------------------------------------------------------------------------------------------------------------
def test_rejected_rows(pa, ctx):
    R = rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    n = 6
    rows = np.arange(n)
    lists = [np.arange(10), np.arange(5, 25), np.array([3, N_ITEM, 4]), np.arange(RC.TOO_LONG) % N_ITEM, np.arange(7), np.arange(40)]
    off, cand = RO.csr(lists)
    good_off = off.copy()
    # row 0 = [5, 0): descending offsets; row 1 then owns [0, 30), the entries of both first lists - no two rows share an entry
    broken = off.copy()
    broken[0], broken[1] = 5, 0
    full = score_rows(pa, m, rows, extra=0)
    for name, o in (("descending", broken), ("past the end", np.concatenate([off[:-1], [len(cand) + 1]]).astype(np.int32))):
        want_s, bad_s = RO.score_lists(full, o, cand)
        got_s = score_lists(pa, m, rows, o, cand)
        assert same_bits(got_s, want_s), name
        assert m.ctx.take_bad_ids() == bad_s and bad_s >= 2, (name, bad_s)          # (row 2 holds an id beyond the table in both)
        want = RO.rerank(o, cand, n, want_s, 20)
        got = fused(pa, m, rows, o, cand, 20)
        assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), name
        # counted once per row whichever stage rejects it: the scoring stage's rows, and the row that is only too long
        rejected = [r for r in range(n) if (got[0][r] == -1).all() and got[3][r] == 0]
        assert m.ctx.take_bad_ids() == len(rejected) == len(set(range(n)) - {r for r in range(n) if want[3][r] > 0}), (name, rejected)
    # the clean offsets: rows 2 (an id beyond the table) and 3 (4097 entries) are rejected, their neighbours untouched
    got = fused(pa, m, rows, good_off, cand, 20)
    assert m.ctx.take_bad_ids() == 2
    for r in (2, 3):
        assert (got[0][r] == -1).all() and np.isneginf(got[1][r]).all() and (got[2][r] == -1).all() and got[3][r] == 0
    for r in (0, 1, 4, 5):
        one = fused(pa, m, rows[r:r + 1], np.array([0, len(lists[r])]), lists[r], 20)
        assert all(np.array_equal(a[0], b[r]) for a, b in zip(one[:1] + one[2:], got[:1] + got[2:])) and same_bits(one[1][0], got[1][r]), r
    assert m.ctx.take_bad_ids() == 0
    # a shared list with an id beyond the table rejects every row, counted once
    sh = np.array([1, 2, N_ITEM + 5, 3])
    assert np.isneginf(score_lists(pa, m, rows, None, sh)).all() and m.ctx.take_bad_ids() == 1
    got = fused(pa, m, rows, None, sh, 3)
    assert (got[0] == -1).all() and (got[3] == 0).all() and m.ctx.take_bad_ids() == 1
    # limits of the host
    import torch
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    f = torch.zeros(4097 * 2, dtype=torch.float32, device="cuda")
    c = dev_ids(np.zeros(4097, np.int32))
    for k in (0, 4097):
        assert ctx.lib.poi_rerank_lists(ctx.handle, None, p(c), 2, 8, p(f), None, 1.0, 0.0, k, p(z), None, None, None, None) == ENOTSUP, k
    assert ctx.lib.poi_rerank_lists(ctx.handle, None, p(c), 2, 4097, p(f), None, 1.0, 0.0, 5, p(z), None, None, None, None) == ENOTSUP
    assert ctx.lib.poi_rerank_lists(ctx.handle, None, p(c), 0, 8, p(f), None, 1.0, 0.0, 5, p(z), None, None, None, None) == 0      # n = 0: a no-op
    assert (z == 0).all()


# ---- 7: the Python layer ----------------------------------------------------------------------------------------------------------------------
def python_layer_checks(m, rows, n_item, tag):
    """rerank over the model's own candidates returns them; weights (0, 1) return the prior's order; score_lists is the listed columns."""
    import torch
    k = min(100, n_item)
    idx, sc = m.compute_sub_candidates(rows, k, return_scores=True)
    got = m.rerank(rows, idx, k, return_scores=True, return_positions=True, return_counts=True)
    assert torch.equal(got[0], idx), tag
    assert same_bits(got[1].cpu().numpy(), sc.cpu().numpy() + np.float32(0.0)), tag
    live = (idx >= 0).sum(1).int()
    assert torch.equal(got[3], live), tag
    assert torch.equal(got[2], torch.where(idx >= 0, torch.arange(k, device=idx.device, dtype=torch.int32)[None, :].expand_as(idx), torch.full_like(idx, -1))), tag
    # the prior's order: distinct priors, descending along the reversed list
    n = idx.shape[0]
    prior = torch.arange(k, device=idx.device, dtype=torch.float32)[None, :].repeat(n, 1)
    back = m.rerank(rows, idx, k, prior=prior, weights=(0.0, 1.0), return_positions=True)
    want_pos = torch.arange(k - 1, -1, -1, device=idx.device, dtype=torch.int32)[None, :].repeat(n, 1)
    full = (idx >= 0).all(1)
    assert full.any() and torch.equal(back[1][full], want_pos[full]) and torch.equal(back[0][full], idx[full].flip(1)), tag
    s = m.score_lists(rows, idx)
    assert s.shape == idx.shape and same_bits(torch.where(idx >= 0, s, torch.full_like(s, float("-inf"))).cpu().numpy(), sc.cpu().numpy()), tag


def test_python_layer_on_bpr_and_spatial(pa):
    from poi_amd import evaluate as E
    for kind, dim in (("bpr", 20), ("spatial", 128)):
        R = rank_case(kind, dim)
        m = build_rank_model(pa, R)
        python_layer_checks(m, np.arange(N_USER), N_ITEM, kind)
        # device lists are checked by the kernel and reported through sync
        import torch
        bad = torch.full((N_USER, 4), N_ITEM + 1, dtype=torch.int32, device=m.device)
        with pytest.raises(IndexError):
            m.rerank(np.arange(N_USER), bad, 3)
        out = m.rerank(np.arange(N_USER), bad, 3, sync=False)
        assert (out == -1).all() and m.ctx.take_bad_ids() == N_USER
        one = m.rerank(np.arange(N_USER), np.arange(50), 20, return_counts=True)      # one shared list
        assert one[0].shape == (N_USER, 20) and (one[1] == 50).all() and m.ctx.last_plan("lists_path") == 1
    R = rank_case("bpr", 20)
    m = build_rank_model(pa, R)
    se = [np.arange(0, 50), np.arange(50, N_USER)]
    got = E.two_stage_metrics(m, m, se, cands=(100, 1000), ks=(5, 10, 20))
    print(got[100])
    for c in (100, 1000):
        assert got[c]["agreement"] == {5: 1.0, 10: 1.0, 20: 1.0}
        assert got[c]["retriever"] == got[c]["ranker"]
        for k in (5, 10, 20):
            assert got[c]["two_stage"]["recall"][k] == got[c]["ranker"]["recall"][k]
    full = E.full_rank_metrics(m, se, [5, 10, 20], exclude="train")
    assert got[100]["ranker"]["recall"][20] == full["at"][20]["recall"] and abs(got[100]["ranker"]["mrr"] - full["mrr"]) < 1e-12


def test_python_layer_on_carnn_and_sessions(pa):
    import torch
    from tests.test_gpu_group import carnn_model
    m = carnn_model(pa)
    python_layer_checks(m, np.arange(21), 150, "carnn")
    s = m.cell_session(n_slot=21)
    rng = np.random.default_rng(4)
    for t in range(3):
        s.advance(np.arange(20), rng.integers(0, 150, 20))      # slot 20 never checks in
    every = np.arange(21)
    idx, sc, cnt = s.candidates(every, 120, return_scores=True, return_counts=True)
    got = s.rerank(every, idx, 120, return_scores=True, return_counts=True)
    assert torch.equal(got[0], idx) and same_bits(got[1].cpu().numpy(), sc.cpu().numpy() + np.float32(0.0))
    assert (got[0][20] == -1).all() and got[2][20] == 0
    # a spatial session: the session operand path
    from tests import test_gpu_session as TS
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    g = TS.spatial_model(pa, T, TS.spatial_init(32, T))
    ss = g.session(n_slot=T["n_user"])
    slots = np.arange(T["n_user"])
    for t in range(3):
        ss.advance(slots[:-2], T["train"][0][:-2, t])
    idx, sc = ss.candidates(slots, 100, return_scores=True)
    got = ss.rerank(slots, idx, 100, return_scores=True, return_positions=True)
    assert torch.equal(got[0], idx) and same_bits(got[1].cpu().numpy(), sc.cpu().numpy() + np.float32(0.0))
    lists = idx[:, :40].flip(1).contiguous()
    assert torch.equal(ss.rerank(slots, lists, 40), idx[:, :40])
    assert same_bits(ss.score_lists(slots, lists).cpu().numpy(), sc[:, :40].flip(1).cpu().numpy())
    assert g.ctx.take_bad_ids() == 0
