"""-m gpu tests of the route recommendation (Session.recommend_route -> poi_route_expand / poi_route_merge + the session advance): a
beam search over a slot's next POIs must reproduce the float64 oracle of tests/route_oracle.py, which scores every hypothesis by
running the oracle's `predict` on history + path from the float32-rounded tables.  Values (the log-probability of every returned path,
the normaliser) are held to the oracle on every slot; the selection is held to it exactly on the slots whose decisions the oracle alone
finds clear (tests/test_route_cpu.py keeps that share at 75 % or more in every fixture).  The rest states identities of two paths of
the library (regimes, grids, repetition, a slot alone) or edge cases by the definition."""
import numpy as np
import pytest

from tests import route_cases as RC
from tests import route_oracle as RO
from tests.gpu_util import RTOL
from tests.test_gpu_session import geo_problem, gru_init, plain_model, spatial_init, spatial_model

pytestmark = pytest.mark.gpu

DEFAULT_SPLIT_MAX = 8192


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


# ---- models --------------------------------------------------------------------------------------------------------------------------
def build(pa, kind, T, P):
    if kind == "spatial":
        return spatial_model(pa, T, P)
    if kind == "plain":
        return plain_model(pa, T, P)
    from tests.test_gpu_session_cells import model
    return model(pa, kind, T, P)


def session_of(pa, kind, T, P, replay=True):
    m = build(pa, kind, T, P)
    s = m.cell_session() if kind in ("lstm", "rnn") else m.session()
    if replay:
        s.replay(T["off"], T["p_flat"])
    return m, s


def expand_slots(s, b, ex=(None, None), path=None, path_len=0, live=None, counts=False, rows=None):
    """poi_route_expand on the slots' own states, one row per slot."""
    import torch
    ids = torch.arange(s.n_slot, device=s.m.device) if rows is None else torch.as_tensor(rows).to(s.m.device)
    users = s.h.index_select(0, ids).float().contiguous()
    sts = s.sts.index_select(0, ids).contiguous() if s.spatial else None
    lp = s.last_poi.index_select(0, ids).contiguous() if s.spatial else None
    return s._route_expand(users, sts, lp, path, path_len, ex, 1, live, b, return_counts=counts)


def bits(*tensors):
    import torch
    torch.cuda.synchronize()
    return [np.ascontiguousarray(t.cpu().numpy()).reshape(t.shape[0], -1).view(np.uint8) for t in tensors]      # (one row of bytes per row)


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def check_paths_valid(paths, total, n_item, excluded, revisit=False):
    """ids in range, no excluded POI, no revisit, -1 only as a suffix (a dead beam: total -inf), beams by descending total."""
    for s in range(paths.shape[0]):
        for k in range(paths.shape[1]):
            p = paths[s, k]
            live = p >= 0
            n_live = int(live.sum())
            assert live[:n_live].all() and (p[n_live:] == -1).all(), (s, k, p)
            assert (p[:n_live] < n_item).all() and not set(p[:n_live].tolist()) & set(excluded[s]), (s, k, p)
            if not revisit:
                assert len(set(p[:n_live].tolist())) == n_live, (s, k, p)
            assert np.isneginf(total[s, k]) == (n_live < paths.shape[2]), (s, k, p, total[s, k])
        t = total[s]
        assert not np.isnan(t).any() and (t[:-1] >= t[1:]).all(), (s, t)


def check_values(R, hist, paths, total, steplp, T):
    """The returned total (and every step's term) against the oracle's log-probability of that same path."""
    sc = R["scorer"]
    tol = 2 * T * RTOL * max(1.0, R["max_abs"])
    worst = 0.0
    for s in range(paths.shape[0]):
        for k in range(paths.shape[1]):
            if paths[s, k, -1] < 0:
                continue
            lp, terms = RO.path_logp(sc, hist[s], paths[s, k])
            worst = max(worst, abs(lp - total[s, k]))
            assert abs(lp - total[s, k]) <= tol, (s, k, lp, total[s, k], tol)
            if steplp is not None:
                assert np.abs(terms - steplp[s, k]).max() <= tol / T, (s, k, terms, steplp[s, k])
    return worst, tol


# ---- 1, 2, 6: values on every slot, selection on the clear slots -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", RC.FIXTURES)
def test_routes_match_the_oracle(pa, kind, name):
    C, R = RC.problem(kind, name), RC.solve(kind, name)
    T, B, steps = C["T"], C["beam"], C["steps"]
    m, s = session_of(pa, kind, T, C["P"])
    before = bits(*[t for t in (s.h, getattr(s, "c", None), s.sts, s.last_poi, s.steps) if t is not None])
    paths, logp, slp = s.recommend_route(np.arange(T["n_user"]), steps, beam=B, exclude="last", return_step_scores=True)
    after = bits(*[t for t in (s.h, getattr(s, "c", None), s.sts, s.last_poi, s.steps) if t is not None])
    assert same_bits(before, after), "a route is a what-if: the session's own state must not move"
    assert paths.shape == (T["n_user"], B, steps) and logp.shape == (T["n_user"], B) and slp.shape == paths.shape
    assert str(paths.dtype) == "torch.int32" and str(logp.dtype) == "torch.float64"
    paths, logp, slp = paths.cpu().numpy(), logp.cpu().numpy(), slp.cpu().numpy()
    check_paths_valid(paths, logp, T["n_item"], [(h[-1],) for h in C["hist"]])
    worst, tol = check_values(R, C["hist"], paths, logp, slp, steps)
    # the normaliser of the slots' own states, from a direct call
    idx, sc, lse = expand_slots(s, B)
    want = np.array([RO.lse(R["scorer"].scores(h)) for h in C["hist"]])
    err = np.abs(lse.cpu().numpy() - want).max()
    clear = R["clear"]
    print("%s %s: total off by %.2e (bar %.2e), lse by %.2e (bar %.2e), %d of %d slots clear"
          % (kind, name, worst, tol, err, RTOL * max(1.0, R["max_abs"]), clear.sum(), len(clear)))
    assert err <= RTOL * max(1.0, R["max_abs"])
    assert clear.mean() >= RC.CLEAR_MIN
    bad = [u for u in np.nonzero(clear)[0] if not np.array_equal(paths[u], R["paths"][u])]
    assert not bad, "slots %s: routes differ from the oracle's, e.g. %s vs %s" % (bad[:8], paths[bad[0]].tolist(), R["paths"][bad[0]].tolist())


# ---- 3: bit identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("spatial", "d20"), ("plain", "d64"), ("spatial", "d128"), ("spatial", "d256"), ("plain", "small")])
def test_candidate_scores_are_the_rank_kernels_scores(pa, kind, name):
    C = RC.problem(kind, name)
    T = C["T"]
    m, s = session_of(pa, kind, T, C["P"])
    slots = np.arange(T["n_user"])
    ex = m._near_exclusion("last", T["n_user"], s.last_poi.contiguous(), kinds=("last",))
    idx, sc, lse = expand_slots(s, 8, ex=ex)
    rank, rsc = s.rank_of(slots, idx, exclude="last", return_scores=True)
    assert same_bits(bits(sc), bits(rsc)), "a candidate's score must be poi_score_rank's score of the same row and POI, bit for bit"
    assert np.array_equal(rank.cpu().numpy(), np.tile(np.arange(8), (T["n_user"], 1)))
    paths, _ = s.recommend_route(slots, 1, beam=1, exclude="last")
    first = s.rank_of(slots, paths[:, 0, 0].contiguous(), exclude="last")
    assert (first.cpu().numpy() == 0).all()


@pytest.fixture(scope="module")
def wide(pa):
    """Spatial and plain sessions over 2100 POIs - five item blocks of the normaliser - with 40 slots."""
    out = {}
    for kind in ("spatial", "plain"):
        T = geo_problem(91, n_user=40, n_item=2100, n_dist=11, dim=16, len_min=4, len_max=12)
        P = spatial_init(16, T) if kind == "spatial" else gru_init(16, T)
        out[kind] = (T, P) + session_of(pa, kind, T, P)
    return out


@pytest.mark.parametrize("kind", ["spatial", "plain"])
def test_every_regime_and_grid_gives_the_same_bits(pa, wide, kind):
    T, _, m, s = wide[kind]
    slots = np.arange(T["n_user"])
    ctx = m.ctx

    def run():
        ex = m._near_exclusion("last", T["n_user"], s.last_poi.contiguous(), kinds=("last",))
        e = expand_slots(s, 8, ex=ex, counts=True)
        plan = (ctx.last_plan("route_path"), ctx.last_plan("route_splits"))
        return bits(*e, *s.recommend_route(slots, 5, beam=4, return_step_scores=True)), plan

    try:
        ref, plan = run()
        assert plan[0] == 1 and plan[1] >= 1
        again, _ = run()
        assert same_bits(ref, again), "a repeated call must give the same bits"
        seen = {}
        for grid in (1, 3, 64):
            ctx.set_option("route_grid", grid)
            got, plan = run()
            seen[grid] = plan
            assert plan == (1, grid) and same_bits(ref, got), "route_grid %d" % grid
        ctx.set_option("route_grid", 0)
        ctx.set_option("route_split_max", 0)
        got, plan = run()
        assert plan == (0, 0) and same_bits(ref, got), "the tile path must give the bits of the split path"
        ctx.set_option("route_split_max", 1 << 30)
        got, plan = run()
        assert plan[0] == 1 and same_bits(ref, got)
    finally:
        ctx.set_option("route_grid", 0)
        ctx.set_option("route_split_max", DEFAULT_SPLIT_MAX)
    # a slot alone
    ex = m._near_exclusion("last", T["n_user"], s.last_poi.contiguous(), kinds=("last",))
    all_e = bits(*expand_slots(s, 8, ex=ex))
    all_r = bits(*s.recommend_route(slots, 5, beam=4, return_step_scores=True))
    for u in (0, 17, 39):
        lp = s.last_poi[u:u + 1].contiguous()
        one_e = bits(*expand_slots(s, 8, ex=m._near_exclusion("last", 1, lp, kinds=("last",)), rows=[u]))
        assert same_bits(one_e, [a[u:u + 1] for a in all_e]), u
        one_r = bits(*s.recommend_route([u], 5, beam=4, return_step_scores=True))
        assert same_bits(one_r, [a[u:u + 1] for a in all_r]), u
    for ctxopt in (0, 1 << 30):                     # ... in either regime
        try:
            ctx.set_option("route_split_max", ctxopt)
            one_r = bits(*s.recommend_route([17], 5, beam=4, return_step_scores=True))
            assert same_bits(one_r, [a[17:18] for a in all_r])
        finally:
            ctx.set_option("route_split_max", DEFAULT_SPLIT_MAX)


def test_wide_routes_match_the_oracle_values(pa, wide):
    """Five item blocks: the normaliser's block order against the oracle's plain sum."""
    from tests.test_gpu_session import seqs_of
    for kind in ("spatial", "plain"):
        T, P, m, s = wide[kind]
        hist = [tuple(int(v) for v in q) for q in seqs_of(T)][:6]
        sc = RO.Scorer(kind, P, T)
        want = np.array([RO.lse(sc.scores(h)) for h in hist])
        paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route(np.arange(6), 3, beam=3, return_step_scores=True))
        check_paths_valid(paths, logp, T["n_item"], [(h[-1],) for h in hist])
        worst, tol = check_values(dict(scorer=sc, max_abs=sc.max_abs), hist, paths, logp, slp, 3)
        _, _, lse = expand_slots(s, 3, rows=list(range(6)))
        err = np.abs(lse.cpu().numpy() - want).max()
        print("wide %s: total off by %.2e (bar %.2e), lse by %.2e" % (kind, worst, tol, err))
        assert err <= RTOL * max(1.0, sc.max_abs)


# ---- 4: edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "plain"])
def test_fresh_slot(pa, kind):
    C = RC.problem(kind, "d20")
    T = C["T"]
    m, s = session_of(pa, kind, T, C["P"], replay=False)
    paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route([0, 5], 1, beam=4, exclude=None, return_step_scores=True))
    assert np.array_equal(paths[:, :, 0], np.tile(np.arange(4), (2, 1))), "all scores are 0 at step 0: the lowest ids, ascending"
    assert np.abs(slp[:, :, 0] + np.log(T["n_item"])).max() <= 4e-15 * np.log(T["n_item"]) and np.array_equal(logp, slp[:, :, 0])
    paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route([0, 5], 3, beam=4, exclude=None, return_step_scores=True))
    assert set(paths[:, :, 0].ravel().tolist()) <= {0, 1, 2, 3} and np.abs(slp[:, :, 0] + np.log(T["n_item"])).max() <= 4e-15 * np.log(T["n_item"])
    sc = RO.Scorer(kind, C["P"], T)
    check_paths_valid(paths, logp, T["n_item"], [(), ()])
    check_values(dict(scorer=sc, max_abs=sc.max_abs), [(), ()], paths, logp, slp, 3)
    st = s.state([0, 5])
    assert (st["last_poi"] == -1).all() and (st["steps"] == 0).all() and not st["h"].any()


def test_candidates_run_out(pa):
    T = geo_problem(5, n_user=6, n_item=10, n_dist=11, dim=8, len_min=4, len_max=12)
    P = gru_init(8, T)
    m, s = session_of(pa, "plain", T, P)
    paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route(np.arange(6), 12, beam=3, exclude="last", return_step_scores=True))
    assert (paths[:, :, :9] >= 0).all() and (paths[:, :, 9:] == -1).all() and np.isneginf(logp).all() and np.isneginf(slp[:, :, 9:]).all()
    last = s.last_poi.cpu().numpy()
    for u in range(6):
        for k in range(3):
            assert sorted(paths[u, k, :9].tolist()) == sorted(set(range(10)) - {int(last[u])}), (u, k, paths[u, k])
    # the same search cut before the candidates run out, against the oracle's values
    hist = [tuple(int(v) for v in T["train"][0][u, :L]) for u, L in enumerate(T["lens"])]
    sc = RO.Scorer("plain", P, T)
    p9, l9, s9 = (t.cpu().numpy() for t in s.recommend_route(np.arange(6), 9, beam=3, exclude="last", return_step_scores=True))
    assert np.array_equal(p9, paths[:, :, :9])
    check_paths_valid(p9, l9, 10, [(h[-1],) for h in hist])
    for h in hist:
        sc.scores(h)
    check_values(dict(scorer=sc, max_abs=sc.max_abs), hist, p9, l9, s9, 9)
    # counts: |C(r)| = n_item - |list union path|
    import torch
    path = torch.tensor([[3, 7, 1, -1]] * 6, dtype=torch.int32, device=m.device)
    eo = torch.tensor([0, 0, 2, 4, 4, 9, 19], dtype=torch.int32, device=m.device)
    lists = [[], [1, 2], [3, 7], [], [0, 2, 4, 6, 8], list(range(10))]
    ei = torch.tensor(sum(lists, []), dtype=torch.int32, device=m.device)
    idx, scv, lse, cnt = expand_slots(s, 3, ex=(eo, ei), path=path, path_len=3, counts=True)
    want = [10 - len(set(l) | {3, 7, 1}) for l in lists]
    assert cnt.cpu().numpy().tolist() == want
    idx = idx.cpu().numpy()
    for u, l in enumerate(lists):
        got = idx[u][idx[u] >= 0]
        assert len(got) == min(3, want[u]) and not set(got.tolist()) & (set(l) | {3, 7, 1}), (u, idx[u])
    assert m.ctx.take_bad_ids() == 0


@pytest.mark.parametrize("kind", ["spatial", "plain"])
def test_exclusion_lists_and_revisits(pa, kind):
    C, R0 = RC.problem(kind, "d20"), RC.solve(kind, "d20")
    T, N = C["T"], C["T"]["n_item"]
    m, s = session_of(pa, kind, T, C["P"])
    slots = [0, 1, 2, 3]
    lists = [[], sorted(set(range(N)) - {4, 9}), list(range(N)), [5, 6, 7]]
    off = np.r_[0, np.cumsum([len(l) for l in lists])]
    paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route(slots, 3, beam=2, exclude=(off, np.array(sum(lists, []), np.int64)), return_step_scores=True))
    sc = R0["scorer"]
    for u in range(4):
        want = RO.beam_search(sc, C["hist"][u], 2, 3, exclude=lists[u])
        assert np.array_equal((paths[u] >= 0), (want["paths"] >= 0)), (u, paths[u], want["paths"])
        if RO.clear(want["gaps"], sc.max_abs):
            assert np.array_equal(paths[u], want["paths"]), (u, paths[u], want["paths"])
    assert sorted(paths[1, 0, :2].tolist()) == [4, 9] and (paths[1, :, 2] == -1).all() and (paths[2] == -1).all() and np.isneginf(logp[2]).all()
    check_paths_valid(paths, logp, N, lists)
    for u in (0, 3):
        check_values(dict(scorer=sc, max_abs=sc.max_abs), [C["hist"][u]], paths[u:u + 1], logp[u:u + 1], slp[u:u + 1], 3)
    # revisit=True: the path is no exclusion
    n = T["n_user"]
    paths, logp, slp = (t.cpu().numpy() for t in s.recommend_route(np.arange(n), 4, beam=3, exclude=None, revisit=True, return_step_scores=True))
    check_paths_valid(paths, logp, N, [()] * n, revisit=True)
    res = [RO.beam_search(sc, h, 3, 4, exclude=(), revisit=True) for h in C["hist"]]
    check_values(dict(scorer=sc, max_abs=sc.max_abs), C["hist"], paths, logp, slp, 4)
    ok = [u for u in range(n) if RO.clear(res[u]["gaps"], sc.max_abs)]
    assert len(ok) >= n // 2
    for u in ok:
        assert np.array_equal(paths[u], res[u]["paths"]), (u, paths[u], res[u]["paths"])


@pytest.mark.parametrize("kind", ["spatial", "plain"])
def test_planted_ties_go_to_the_lower_id(pa, kind):
    n_dist, dim, n_item = 11, 20, 50
    T = geo_problem(7 + dim + n_dist, n_user=8, n_item=n_item, n_dist=n_dist, dim=dim, len_min=4, len_max=12)
    T["coords"][37] = T["coords"][12]
    P = spatial_init(dim, T) if kind == "spatial" else gru_init(dim, T)
    P["lt"][37] = P["lt"][12]
    m, s = session_of(pa, kind, T, P)
    import torch
    keep = {12, 37, 3, 20, 41}                       # everything else is excluded: both twins are in every list
    lst = sorted(set(range(n_item)) - keep)
    eo = torch.arange(9, dtype=torch.int32, device=m.device) * len(lst)
    ei = torch.tensor(lst * 8, dtype=torch.int32, device=m.device)
    idx, sc, lse, cnt = expand_slots(s, 8, ex=(eo, ei), counts=True)
    idx, scb = idx.cpu().numpy(), sc.cpu().numpy().view(np.uint32)
    assert (cnt.cpu().numpy() == 5).all() and (idx[:, 5:] == -1).all()
    for u in range(8):
        a, b = idx[u].tolist().index(12), idx[u].tolist().index(37)
        assert b == a + 1 and scb[u, a] == scb[u, b], (u, idx[u], sc[u])
    paths, logp = (t.cpu().numpy() for t in s.recommend_route(np.arange(8), 1, beam=5, exclude=(eo, ei)))
    assert np.array_equal(paths[:, :, 0], idx[:, :5])


def test_merge_order_and_dead_proposals(pa):
    import torch
    C = RC.problem("plain", "d20")
    m, s = session_of(pa, "plain", C["T"], C["P"], replay=False)
    dev = m.device
    inf, nan = float("inf"), float("nan")
    B, P = 3, 3
    # slot 0: equal totals across parents and inside a parent; slot 1: -inf / NaN proposals and a dead parent; slot 2: one live proposal
    idx = torch.tensor([[[7, 2, 9], [2, 7, 5], [1, 4, 6]],
                        [[3, 8, -1], [5, 6, 7], [9, 9, 9]],
                        [[4, -1, -1], [1, 2, 3], [1, 2, 3]]], dtype=torch.int32, device=dev)
    score = torch.tensor([[[1.0, 1.0, 0.5], [2.0, 2.0, 0.0], [1.0, 0.25, 0.0]],
                          [[1.0, -inf, 0.0], [nan, 0.5, 0.25], [9.0, 9.0, 9.0]],
                          [[0.5, 0.0, 0.0], [5.0, 5.0, 5.0], [5.0, 5.0, 5.0]]], dtype=torch.float32, device=dev)
    lse = torch.tensor([[2.0, 3.0, 2.0], [2.0, 2.0, nan], [1.0, 1.0, 1.0]], dtype=torch.float64, device=dev)
    total = torch.tensor([[-1.0, -1.0, -1.0], [-1.0, -0.5, -inf], [-2.0, -1.0, -1.0]], dtype=torch.float64, device=dev)
    n_live = torch.tensor([3, 3, 1], dtype=torch.int32, device=dev)
    parent, poi, tot, slp, nl = s._route_merge(idx.reshape(9, 3).contiguous(), score.reshape(9, 3).contiguous(), lse.reshape(-1).contiguous(),
                                               total, n_live, 3, P, B, return_step_scores=True)
    parent, poi, tot, slp, nl = (t.cpu().numpy() for t in (parent, poi, tot, slp, nl))
    # slot 0: five proposals at total -2 - parent 0 (ids 2 and 7), parent 1 (2 and 7), parent 2 (1): lower parent, then lower id
    assert parent[0].tolist() == [0, 0, 1] and poi[0].tolist() == [2, 7, 2] and tot[0].tolist() == [-2.0, -2.0, -2.0] and slp[0].tolist() == [-1.0, -1.0, -1.0]
    # slot 1: (parent 0, 3) at -2, (parent 1, 6) at -2, (parent 1, 7) at -2.25; the -inf score, the NaN score and the NaN normaliser are dead
    assert parent[1].tolist() == [0, 1, 1] and poi[1].tolist() == [3, 6, 7] and tot[1].tolist() == [-2.0, -2.0, -2.25]
    # slot 2: one live parent with one candidate
    assert poi[2].tolist() == [4, -1, -1] and parent[2].tolist() == [0, 1, 2] and tot[2][0] == -2.5 and np.isneginf(tot[2][1:]).all() and np.isneginf(slp[2][1:]).all()
    assert nl.tolist() == [3, 3, 1]


def test_a_malformed_exclusion_list_kills_its_slot_alone(pa):
    import torch
    C = RC.problem("plain", "d20")
    T = C["T"]
    m, s = session_of(pa, "plain", T, C["P"])
    dev = m.device
    eo = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=dev)
    good = torch.tensor([1, 5, 2, 9, 0, 3], dtype=torch.int32, device=dev)
    bad = torch.tensor([1, 5, 9, 2, 0, 3], dtype=torch.int32, device=dev)       # slot 1's list descends
    ref = [t.cpu().numpy() for t in s.recommend_route([0, 1, 2], 4, beam=3, exclude=(eo, good))]
    assert m.ctx.take_bad_ids() == 0
    got = [t.cpu().numpy() for t in s.recommend_route([0, 1, 2], 4, beam=3, exclude=(eo, bad), sync=False)]
    assert m.ctx.take_bad_ids() == 1, "the row is rejected once: its slot is dead afterwards and is not read again"
    assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()
    for u in (0, 2):
        assert np.array_equal(got[0][u], ref[0][u]) and np.array_equal(got[1][u].view(np.uint64), ref[1][u].view(np.uint64))
    with pytest.raises(IndexError):
        s.recommend_route([0, 1, 2], 4, beam=3, exclude=(eo, bad))
    out_of_range = torch.tensor([1, 5, 2, 50, 0, 3], dtype=torch.int32, device=dev)
    with pytest.raises(IndexError):
        s.recommend_route([0, 1, 2], 2, beam=2, exclude=(eo, out_of_range))


def test_argument_checks_and_carnn(pa):
    C = RC.problem("plain", "d20")
    m, s = session_of(pa, "plain", C["T"], C["P"])
    for steps, beam in ((4, 9), (17, 4), (0, 4)):
        with pytest.raises(pa._lib.PoiError):
            s.recommend_route([0], steps, beam=beam)
    paths, logp = s.recommend_route([3, 3, 0], 2, beam=2)                       # repeated slots are only read
    assert np.array_equal(paths[0].cpu().numpy(), paths[1].cpu().numpy()) and np.array_equal(logp[0].cpu().numpy(), logp[1].cpu().numpy())
    from tests import session_cells_oracle as S
    from tests.test_gpu_session_cells import model
    T = geo_problem(300 + 8 + 11, n_user=6, n_item=50, n_dist=11, dim=8, len_min=4, len_max=12)
    cs = model(pa, "carnn", T, S.carnn_params(8, T)).cell_session()
    with pytest.raises(pa._lib.PoiError, match="OboCARNN"):
        cs.recommend_route([0], 3)
