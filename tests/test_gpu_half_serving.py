"""-m gpu tests of the serving paths on a HALF POI table (table_dtype="f16": `lt` and its snapshot `trained_items` stored as IEEE half,
the storage form of BASELINE's config X).  The kernels decide per launch how to read the table - is_f16(ctx, ptr) sets `lt_f16` /
`items_f16` - and every one of them then takes another load path: ld_tab in both session kernels (session.hip), ld4t in the restricted
top-K (near.hip) and the AUC flags (misc.hip), load_frag at the first tile, the double-buffered prefetch and the single-buffer refill
of group.hip and route.hip.  Every result is held to the float64 oracle run from the table's float16 ROUNDING
(tests/half_cases.py; tests/test_half_cases_cpu.py shows that the oracle from the unrounded float32 init would miss every bar used
here), at the bars of the float32 tests: RTOL on states and values, exact lists on qualifying rows.  Every test first asserts that the
model's snapshot is torch.float16."""
import ctypes
import gc

import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import group_cases as GC
from tests import group_oracle as GO
from tests import half_cases as HC
from tests import near_oracle as NO
from tests import route_cases as RC
from tests import route_oracle as RO
from tests.gpu_util import RTOL, assert_close, rel_err
from tests.test_gpu_near import check, near
from tests.test_gpu_route import DEFAULT_SPLIT_MAX, bits, check_paths_valid, check_values, expand_slots, same_bits
from tests.test_gpu_session import oracle_rows, seqs_of

pytestmark = pytest.mark.gpu

K = HC.K


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def half_model(pa, build):
    import torch
    m = build(pa)
    assert m.trained_items.t.dtype == torch.float16 and m.lt.t.dtype == torch.float16
    return m


def replayed(pa, C, n_slot=None):
    m = half_model(pa, C["build"])
    s = m.session(n_slot)
    s.replay(C["T"]["off"], C["T"]["p_flat"])
    return m, s


def check_state(C, st, hts, sts, what):
    """h (and sts) within RTOL of the oracle's; -> the worse of the two errors as a fraction of RTOL."""
    e = assert_close(st["h"], hts, "h " + what)
    if C["spatial"]:
        e = max(e, assert_close(st["sts"], sts, "sts " + what))
    else:
        assert "sts" not in st
    return e / RTOL


# ---- 1: replay == predict ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.SESSION_CASES))
def test_replay_equals_predict(pa, name):
    C = HC.session_case(name)
    T = C["T"]
    m, s = replayed(pa, C)
    st = s.state()
    err = [rel_err(st["h"], C["hts"])] + ([rel_err(st["sts"], C["sts"])] if C["spatial"] else [])
    print("half replay %s: worst state error %.2e of RTOL" % (name, max(err) / RTOL))
    check_state(C, st, C["hts"], C["sts"], name)
    assert np.array_equal(st["last_poi"], [q[-1] for q in seqs_of(T)]) and np.array_equal(st["steps"], T["lens"])
    if name == "plain20":                                # stored padded: the pad columns of the table and of the state stay exactly zero
        assert m.kdim == 64 and s.h.shape[1] == 64 and float(s.h[:, 20:].abs().max()) == 0.0
        assert float(m.trained_items.t[:, 20:].float().abs().max()) == 0.0
    else:
        assert m.kdim == T["dim"]


# ---- 2: both advance kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.ADVANCE_CASES)
def test_both_advance_kernels(pa, name):
    A = HC.advance_case(name)
    C = A["C"]
    T = C["T"]
    n = T["n_user"]
    m = half_model(pa, C["build"])
    default = None
    out = {}
    try:
        for tile_min, path in ((1, 1), (1 << 30, 0)):
            s = m.session()
            s.replay(T["off"], T["p_flat"])
            default = m.ctx.last_plan("session_tile_min") if default is None else default
            m.ctx.set_option("session_tile_min", tile_min)
            s.advance(np.arange(n), A["ev"])
            assert m.ctx.last_plan("session_path") == path and m.ctx.last_plan("session_tile_min") == tile_min
            assert m.ctx.last_plan("session_tiles") == ((n + 15) // 16 if path else 0)
            m.ctx.set_option("session_tile_min", default)
            st = s.state()
            e = check_state(C, st, A["h1"], A["s1"], "%s, session_path %d" % (name, path))
            print("half advance %s, session_path %d: worst state error %.2e of RTOL" % (name, path, e))
            assert np.array_equal(st["last_poi"], A["ev"]) and np.array_equal(st["steps"], T["lens"] + 1)
            out[path] = st
    finally:
        if default is not None:
            m.ctx.set_option("session_tile_min", default)
    assert default == 512 and rel_err(out[0]["h"], out[1]["h"]) <= 2 * RTOL


# ---- 3: the session reads the snapshot, not the live table -----------------------------------------------------------------------------
def test_session_follows_the_snapshot(pa):
    C = HC.session_case("plain64")
    T, P = C["T"], C["Ph"]
    m = half_model(pa, C["build"])
    users = np.arange(T["n_user"], dtype=np.int32)
    for _ in range(3):
        m.train_batch(users)
    par = {k: np.float64(getattr(m, k).get_value()) for k in ("lt", "ui", "wh", "bi")}
    assert getattr(m, "lt").get_value().dtype == np.float16 and np.abs(par["lt"] - P["lt"]).max() > 0
    new = {**P, **par}
    old = {**new, "lt": P["lt"]}                         # the snapshot still holds the initial half table; ui / wh / bi are live
    h_old, _ = oracle_rows(old, T, seqs_of(T), spatial=False)
    h_new, _ = oracle_rows(new, T, seqs_of(T), spatial=False)
    assert rel_err(h_old, h_new) > 10 * RTOL, "the steps moved the table by too little to tell the two snapshots apart"
    s = m.session()
    s.replay(T["off"], T["p_flat"])
    assert_close(s.state()["h"], h_old, "h on the old snapshot")
    m.update_trained_items()
    s = m.session()                                      # a fresh replay
    s.replay(T["off"], T["p_flat"])
    e = assert_close(s.state()["h"], h_new, "h on the new snapshot")
    print("half replay after %d steps: worst state error %.2e of RTOL" % (3, e / RTOL))
    assert np.array_equal(np.float64(m.trained_items.get_value()), par["lt"]) and np.array_equal(np.float64(m.lt.get_value()), par["lt"])


# ---- 4: Session.recommend -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.RECOMMEND_CASES))
def test_session_recommend(pa, name):
    import torch
    C = HC.recommend_case(name)
    T = C["T"]
    m, s = replayed(pa, C)
    check_state(C, s.state(), C["hts"], C["sts"], "recommend " + name)
    slots = np.arange(T["n_user"])
    mask = np.ones_like(C["sc"], bool)
    cnt = torch.full((T["n_user"],), T["n_item"], dtype=torch.int32)
    for k in HC.RECOMMEND_K:                             # 40: explicit score rows (poi_score_all on the half table) + poi_topk
        idx, sc = s.recommend(slots, k, return_scores=True)
        check((idx, sc, cnt), C["sc"], mask, k, "half recommend %s k %d" % (name, k))


# ---- 5: restricted top-K ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", HC.RANK_CASES)
def test_near_on_both_paths(pa, kind, dim):
    import torch
    R = HC.near_case(kind, dim)
    C = R["C"]
    m = half_model(pa, C["build"])
    assert m.kdim == dim
    rows = np.arange(HC.NEAR_USERS)
    default = 256
    try:
        for r_km in HC.NEAR_RADII:
            ref = None
            for split_max, grid in ((0, 0), (1 << 30, 3)):
                m.ctx.set_option("near_split_max", split_max); m.ctx.set_option("near_grid", grid)
                out = near(m, rows, within_km=r_km, exclude=R["ex"])
                plan = {k: m.ctx.last_plan(k) for k in ("near_path", "near_splits", "near_split_max")}
                assert plan == (dict(near_path=1, near_splits=grid, near_split_max=1 << 30) if split_max else dict(near_path=0, near_splits=0, near_split_max=0)), plan
                idx, sc, cnt = check(out, R["sc"], R["masks"][r_km], K, "half near %s dim %d, %s km, path %d" % (kind, dim, r_km, plan["near_path"]))
                assert cnt[3] == 0 and np.all(idx[3] == -1)
                ref = ref or out
                assert all(torch.equal(a, b) for a, b in zip(out, ref)), "the two paths differ"
    finally:
        m.ctx.set_option("near_split_max", default); m.ctx.set_option("near_grid", 0)
    assert m.ctx.take_bad_ids() == 0


# ---- 6: group recommendation -----------------------------------------------------------------------------------------------------------
def group_rec(m, off, ids, **kw):
    return m.recommend_group((off, ids), K, return_scores=True, return_counts=True, **kw)


@pytest.mark.parametrize("kind,dim", HC.RANK_CASES)
def test_group_in_both_regimes(pa, kind, dim):
    import torch
    R = HC.group_case(kind, dim)
    m = half_model(pa, R["C"]["build"])
    if kind == "spatial":
        m._last_poi[list(GC.NO_LAST)] = -1               # (as tests/test_gpu_group.py: these members have no distance term)
    assert m.kdim == dim
    off, ids = R["off"], R["ids"]
    keys = ("group_path", "group_splits", "group_split_max")
    default = 256
    try:
        for agg in GO.AGGS:
            for name, ex in (("", (None, None)), (", lists", R["ex"])):
                a, mask = GO.aggregate(R["sc"], off, ids, agg), GO.candidate_mask(off, R["sc"].shape[1], ex[0], ex[1])
                ref = None
                for split_max, grid in ((0, 0), (1 << 30, 1), (1 << 30, 3)):
                    m.ctx.set_option("group_split_max", split_max); m.ctx.set_option("group_grid", grid)
                    out = group_rec(m, off, ids, agg=agg, exclude=None if ex[0] is None else ex)
                    plan = {k: m.ctx.last_plan(k) for k in keys}
                    assert plan == (dict(group_path=1, group_splits=grid, group_split_max=1 << 30) if split_max else dict(group_path=0, group_splits=0, group_split_max=0)), plan
                    idx, sc, cnt = check(out, a, mask, K, "half group %s dim %d %s%s, path %d grid %d" % (kind, dim, agg, name, plan["group_path"], grid))
                    assert cnt[9] == 0 and np.all(idx[9] == -1)      # the empty group
                    ref = ref or out
                    assert all(torch.equal(x, y) for x, y in zip(out, ref)), "the regimes differ"
    finally:
        m.ctx.set_option("group_split_max", default); m.ctx.set_option("group_grid", 0)
    assert m.ctx.take_bad_ids() == 0


def test_session_recommend_group(pa):
    S = HC.session_group_case()
    C = S["C"]
    T, P = C["T"], C["Ph"]
    m = half_model(pa, C["build"])
    s = m.session(n_slot=S["n_slot"])
    for t in range(3):                                   # three check-ins per slot; the last two slots never check in
        s.advance(np.arange(T["n_user"]), T["train"][0][:, t])
    st = s.state()
    hts, _ = oracle_rows(P, T, S["seqs"], spatial=False)
    assert_close(st["h"][:-2], hts, "h after three check-ins")
    assert np.array_equal(st["last_poi"][-2:], [-1, -1]) and not st["h"][-2:].any()
    msc = GO.member_scores(np.float64(np.float32(st["h"])), P["lt"])      # the kernel reads the float32 rounding of the state
    mask = GO.candidate_mask(S["off"], T["n_item"], *S["ex"])
    for agg in GO.AGGS:
        out = s.recommend_group((S["off"], S["ids"]), K, agg=agg, exclude=S["ex"], return_scores=True, return_counts=True)
        check(out, GO.aggregate(msc, S["off"], S["ids"], agg), mask, K, "half session group %s" % agg)


# ---- 7: routes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", HC.ROUTE_CASES)
def test_routes_match_the_oracle_in_both_regimes(pa, kind, name):
    C = HC.route_case(kind, name)
    T, B, steps = C["T"], C["beam"], C["steps"]
    n = T["n_user"]
    m, s = replayed(pa, C)
    ctx = m.ctx
    state = lambda: bits(*[t for t in (s.h, s.sts, s.last_poi, s.steps) if t is not None])
    before = state()
    ref = None
    try:
        for split_max in (0, 1 << 30):
            ctx.set_option("route_split_max", split_max)
            out = s.recommend_route(np.arange(n), steps, beam=B, exclude="last", return_step_scores=True)
            assert ctx.last_plan("route_path") == (1 if split_max else 0)
            if n * B >= 512:                             # the hypothesis rows' advance took sess_tile_kernel
                assert (kind, name) == HC.TILE_ADVANCE and ctx.last_plan("session_path") == 1 and ctx.last_plan("session_tiles") == (n * B + 15) // 16
            else:
                assert ctx.last_plan("session_path") == 0
            ref = ref or bits(*out)
            assert same_bits(bits(*out), ref), "the tile path must give the bits of the split path"
            idx, sc, lse = expand_slots(s, B)
            assert same_bits(state(), before), "a route is a what-if: the session's own state must not move"
            paths, logp, slp = (t.cpu().numpy() for t in out)
            assert paths.shape == (n, B, steps) and logp.shape == (n, B) and slp.shape == paths.shape
            check_paths_valid(paths, logp, T["n_item"], [(h[-1],) for h in C["hist"]])
            worst, tol = check_values(C, C["hist"], paths, logp, slp, steps)
            want = np.array([RO.lse(C["scorer"].scores(h)) for h in C["hist"]])
            err = np.abs(lse.cpu().numpy() - want).max()
            clear = C["clear"]
            print("half route %s %s, route_path %d: total off by %.2e (bar %.2e), lse by %.2e (bar %.2e), %d of %d slots clear"
                  % (kind, name, 1 if split_max else 0, worst, tol, err, RTOL * max(1.0, C["max_abs"]), clear.sum(), len(clear)))
            assert err <= RTOL * max(1.0, C["max_abs"])
            assert clear.mean() >= RC.CLEAR_MIN
            bad = [u for u in np.nonzero(clear)[0] if not np.array_equal(paths[u], C["paths"][u])]
            assert not bad, "slots %s: routes differ from the oracle's, e.g. %s vs %s" % (bad[:8], paths[bad[0]].tolist(), C["paths"][bad[0]].tolist())
    finally:
        ctx.set_option("route_split_max", DEFAULT_SPLIT_MAX)
    assert ctx.take_bad_ids() == 0


# ---- 8: AUC preference flags -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", HC.AUC_CASES)
def test_auc_preference_flags(pa, kind, dim):
    A = HC.auc_case(kind, dim)
    m = half_model(pa, A["C"]["build"])
    assert np.array_equal(m.tes_buys_masks.cpu().numpy(), A["tp"]) and np.array_equal(m.tes_buys_neg_masks.cpu().numpy(), A["tq"])
    flags = m.compute_sub_auc_preference(np.arange(HC.NEAR_USERS))
    assert flags.shape == A["margin"].shape and flags.dtype == bool
    sure = np.abs(A["margin"]) >= 1e-6 * A["scale"]
    assert sure.mean() >= 0.9
    assert np.array_equal(flags[sure], (A["margin"] > 0)[sure])
    pl = A["planted"]                                    # pairs whose sign the half rounding turns: the float32 values would give the other flag
    assert len(pl) == HC.AUC_PLANTED and np.array_equal(flags[pl], (A["margin32"] <= 0)[pl])


# ---- 9: the registry forgets a dropped half model ----------------------------------------------------------------------------------------
def test_a_dropped_half_model_leaves_no_registration(pa):
    import torch
    H, F = HC.hygiene_case()
    users, items = F["users"], F["items"]
    rows = np.arange(HC.NEAR_USERS)
    m = half_model(pa, H["C"]["build"])
    ctx = m.ctx
    check(near(m, rows, exclude=H["ex"]), H["sc"], H["masks"][None], K, "the half model before it is dropped")
    old = m.trained_items.t                               # the snapshot's memory, kept past the model
    span = (old.data_ptr(), old.data_ptr() + 2 * old.numel())
    del m
    gc.collect()
    # a float32 table AT the dropped snapshot's address: 149 POIs and the padding row of the same tables
    n_sub = HC.HYGIENE_SUB
    t32 = old.view(torch.float32).reshape(-1)[:(n_sub + 1) * 20].view(n_sub + 1, 20)
    assert t32.data_ptr() == span[0]
    t32.copy_(torch.as_tensor(np.float32(items[:n_sub + 1])).to(t32.device))
    u32 = torch.as_tensor(np.float32(users)).to(t32.device)
    idx = torch.empty((len(rows), K), dtype=torch.int32, device=t32.device)
    ptr = pa.models._ptr
    ctx.check(ctx.lib.poi_score_topk(ctx.handle, ptr(u32), ptr(t32), len(rows), n_sub, 20, None, None, K, ptr(idx), None,
                                     ctypes.c_void_p(torch.cuda.current_stream(t32.device).cuda_stream)))
    sub = NO.scores(users, items[:n_sub + 1])
    ok = NO.qualifying(sub, np.ones_like(sub, bool), K)
    assert ok.mean() >= 0.9 and np.array_equal(idx.cpu().numpy()[ok], O.topk_desc(sub, K)[ok]), "a float32 table at the dropped table's address is read as half"
    del t32, old
    # ... and a float32 model of the same shapes ranks by the UNROUNDED table
    f = F["build"](pa)
    assert f.trained_items.t.dtype == torch.float32 and f.ctx is ctx
    at = f.trained_items.t.data_ptr()
    print("the float32 snapshot %s the dropped half snapshot's memory" % ("overlaps" if at < span[1] and at + 4 * f.trained_items.t.numel() > span[0] else "lies beside"))
    sc = NO.scores(users, items)
    mask = np.ones_like(sc, bool)
    out = f.compute_sub_topk(rows, K, return_scores=True)
    check(out + (torch.full((len(rows),), HC.N_ITEM, dtype=torch.int32),), sc, mask, K, "the float32 model after the half model")
    check(near(f, rows, exclude=H["ex"]), sc, H["masks"][None], K, "the float32 model after the half model, restricted")
