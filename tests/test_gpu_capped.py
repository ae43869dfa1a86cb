"""-m gpu tests of the capped recommendation (poi_labels_build, poi_score_topk_capped, poi_topk_capped_scores ->
models.poi_labels / compute_sub_topk_capped, Session.recommend_capped).  The fill table and the explicit-score entry are held EXACTLY
to the numpy oracle of tests/capped_oracle.py on the fixtures of tests/filter_cases.py and tests/capped_cases.py; the fused walk
exactly to the oracle applied to the matrix poi_score_rows writes, and - where the cap cannot bind - bit for bit to the existing
filtered entries; planted tables with exact products check the ties and the merges; every grid, regime and call size gives the same
bits; and both entries, independently of the project's own score rows, equal the float64 oracle on the rows with clear gaps."""
import ctypes

import numpy as np
import pytest

from tests import capped_cases as CC
from tests import capped_oracle as CO
from tests import filter_cases as FC
from tests import filter_oracle as FO
from tests.gpu_util import RTOL
from tests.test_gpu_filter import Fused, dev, dev_ex, dev_u32, filtered_scores, p, same_bits, sub_lists, untrusted_words

pytestmark = pytest.mark.gpu

WALK = 1
EINVAL, ENOTSUP = -1, -4
BIG = 1 << 30


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
    c.set_option("capped_split_max", 256); c.set_option("capped_grid", 0)


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: ids differ on rows %s" % (what, np.nonzero((got[0] != want[0]).any(axis=1))[0][:8])
    assert same_bits(got[1], want[1]), "%s: scores differ" % what
    assert np.array_equal(got[2], want[2]), "%s: labels differ" % what
    assert np.array_equal(got[3], want[3]), "%s: counts %s vs %s" % (what, got[3][:8], want[3][:8])


def cut(want, k):
    return want[0][:, :k], want[1][:, :k], want[2][:, :k], want[3]


def out_buffers(n, k):
    import torch
    k = max(k, 1)
    return (torch.full((n, k), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), 7.0, dtype=torch.float32, device="cuda"),
            torch.full((n, k), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"))


def to_host(bufs):
    return tuple(t.cpu().numpy() for t in bufs)


# ---- 1: poi_labels_build ---------------------------------------------------------------------------------------------------------------
def labels_build(ctx, lab, n_label, words=None, counts=True):
    """poi_labels_build -> (fill (rows, 33), counts (n_label) or None, rejected POIs, the fill tensor); the buffers start as -7."""
    import torch
    n_item = len(lab)
    rows = 1 if words is None else words.shape[0]
    fill = torch.full((rows, 33), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n_label,), -7, dtype=torch.int32, device="cuda") if counts else None
    d_lab = dev(np.asarray(lab, np.int32))
    ctx.check(ctx.lib.poi_labels_build(ctx.handle, p(d_lab), n_item, n_label, p(words), 0 if words is None else words.shape[1],
                                       0 if words is None else rows, p(cnt), p(fill), None))
    bad = ctx.take_bad_ids()
    return fill.cpu().numpy(), (cnt.cpu().numpy() if counts else None), bad, fill


@pytest.mark.parametrize("n_item", [1, 32, 65, 1003])
def test_fill_and_counts_are_the_oracle(ctx, n_item):
    cat, flags = FC.attributes()
    pmask, _ = FO.pass_mask(cat[:n_item], flags[:n_item], FC.N_CAT, FC.PREDICATES)
    words = dev_u32(untrusted_words(pmask))                          # two pad words, every bit at j >= n_item set
    for name in CC.LABELINGS:
        full, n_full = CC.labeling(name, FC.N_ITEM)
        lab = full[:n_item]
        for n_label in sorted({min(n_full, n_item), min(max(n_full // 2, 1), n_item)}):      # the second: the upper labels are strays
            for w, pm in ((None, None), (words, pmask)):
                want = CO.fill_table(lab, n_label, pm)
                fill, cnt, bad, _ = labels_build(ctx, lab, n_label, w)
                assert np.array_equal(fill, want[0]), (name, n_item, n_label, w is None)
                assert np.array_equal(cnt, want[1]) and bad == want[2], (name, n_item, n_label, bad, want[2])
    assert labels_build(ctx, lab, n_label, None, counts=False)[1] is None
    z = dev(np.zeros(64, np.int32))
    assert ctx.lib.poi_labels_build(ctx.handle, p(z), 64, 0, None, 0, 0, None, p(z), None) == EINVAL          # n_label < 1
    assert ctx.lib.poi_labels_build(ctx.handle, p(z), 8, 9, None, 0, 0, None, p(z), None) == EINVAL           # n_label > n_item
    assert ctx.lib.poi_labels_build(ctx.handle, p(z), 64, 1, p(z), 1, 1, None, p(z), None) == EINVAL          # ldw 1 < 2
    assert ctx.lib.poi_labels_build(ctx.handle, None, 64, 1, None, 0, 0, None, p(z), None) == EINVAL


def test_many_predicates_go_through_the_histogram_workspace_in_chunks(ctx):
    """Option "capped_hist_kb": 11 predicates x 1004 ints are 43 KiB - 1 KiB holds one predicate at a time, 8 KiB two (five chunks and
    a ragged one); the tables, the counts and the strays (counted ONCE, not once per chunk) do not depend on it."""
    cat, flags = FC.attributes()
    pmask, _ = FO.pass_mask(cat, flags, FC.N_CAT, FC.PREDICATES)
    words = dev_u32(untrusted_words(pmask))
    try:
        for name, n_label in (("distinct", 1003), ("distinct", 501), ("zipf", 20)):
            lab = CC.labeling(name, FC.N_ITEM)[0]
            want = CO.fill_table(lab, n_label, pmask)
            for kb in (1, 8, 256 << 10):
                ctx.set_option("capped_hist_kb", kb)
                fill, cnt, bad, _ = labels_build(ctx, lab, n_label, words)
                assert np.array_equal(fill, want[0]) and np.array_equal(cnt, want[1]) and bad == want[2], (name, n_label, kb, bad, want[2])
        assert want[2] > 0
    finally:
        ctx.set_option("capped_hist_kb", 256 << 10)


# ---- 2: poi_topk_capped_scores on the planted rows ------------------------------------------------------------------------------------
def capped_scores(ctx, sc, n_item, lab, per, k, fill=None, words=None, pred=None, ex=(None, None), expect=0):
    n = sc.shape[0]
    bufs = out_buffers(n, k)
    rc = ctx.lib.poi_topk_capped_scores(ctx.handle, p(sc), n, n_item, sc.shape[1], p(lab), per, p(fill), p(words), 0 if words is None else words.shape[1],
                                        0 if words is None else words.shape[0], p(pred), p(ex[0]), p(ex[1]), k, p(bufs[0]), p(bufs[1]), p(bufs[2]),
                                        p(bufs[3]), None)
    if expect:
        assert rc == expect, (rc, expect)
        return rc
    ctx.check(rc)
    return to_host(bufs)


@pytest.mark.parametrize("name", CC.LABELINGS)
@pytest.mark.parametrize("shape", list(FC.SCORE_SHAPES))
def test_explicit_scores_are_the_oracle_on_every_row(ctx, shape, name):
    from tests.select_cases import padded
    F = FC.score_fixture(shape)
    n, N = F["sc"].shape
    lab, n_label = CC.labeling(name, N)
    mask, bad = FO.candidate_masks(F["pmask"], F["pred"], n, *F["ex"])
    sc = dev(padded(F["sc"]))                                        # three more columns of 1e30: ld > n_item, never read
    words = dev_u32(untrusted_words(F["pmask"]))
    pred, ex, d_lab = dev(F["pred"].astype(np.int32)), dev_ex(F["ex"]), dev(lab)
    fill = dev(CO.fill_table(lab, n_label, F["pmask"])[0])
    for per in CC.PER_SET:
        want = CO.topk(F["sc"], mask, lab, per, 32)
        for k in CC.K_SET:
            got = capped_scores(ctx, sc, N, d_lab, per, k, fill, words, pred, ex)
            assert_same(got, cut(want, k), "%s %s per %d k %d" % (shape, name, per, k))
            assert ctx.take_bad_ids() == int(F["bad"].sum())         # every bad row counted once
            if per == 32 or name == "distinct":                      # the cap cannot bind: the filtered entry, bit for bit
                ref = filtered_scores(ctx, sc, N, words, pred, ex, k)
                assert np.array_equal(got[0], ref[0]) and same_bits(got[1], ref[1]) and np.array_equal(got[3], ref[2])
                assert ctx.take_bad_ids() == int(F["bad"].sum())
    # bits NULL: every POI passes, pred is ignored (the two rows with a bad predicate index are good rows now); no lists, no fill
    got = capped_scores(ctx, sc, N, d_lab, 2, 20, None, None, pred, (None, None))
    assert_same(got, CO.topk(F["sc"], np.ones((n, N), bool), lab, 2, 20), "%s %s bits NULL" % (shape, name))
    assert ctx.take_bad_ids() == 0


# ---- the fused walk ---------------------------------------------------------------------------------------------------------------------
def capped_call(U, lab, per, k=FC.K, rows=None, pred="own", ex="own", fill=None, bits=True, anchor="own", expect=0, n_arg=None, users=None, dim=None):
    """poi_score_topk_capped on the rows `rows` of a Fused case (default: all) -> (ids, scores, labels, counts) numpy, or the error
    code.  fill: None, or a device tensor whose rows the predicates index."""
    m, F = U.m, U.F
    rows = np.arange(U.n) if rows is None else np.asarray(rows)
    sel = dev(rows.astype(np.int64))
    n = len(rows)
    usr = U.users.index_select(0, sel).contiguous() if users is None else users
    wd, sts, thr, n_dist, dd_m = U.term if U.term is not None else (None, None, None, 0, 0.0)
    sts = None if sts is None else sts.index_select(0, sel).contiguous()
    anc = U.anchor.index_select(0, sel).contiguous() if isinstance(anchor, str) else anchor
    prd = dev(F["pred"][rows].astype(np.int32)) if isinstance(pred, str) else (None if pred is None else dev(np.asarray(pred, np.int32)))
    exd = dev_ex(sub_lists(F["ex"], rows) if isinstance(ex, str) else ex)
    words = U.words if bits is True else bits
    bufs = out_buffers(n, k)
    rc = m.lib.poi_score_topk_capped(m.ctx.handle, p(usr), p(U.items), n if n_arg is None else n_arg, U.N, m.kdim if dim is None else dim, p(wd), p(sts),
                                     p(U.geo[0]), p(U.geo[1]), p(thr), p(anc), int(n_dist), float(dd_m), p(lab), per, p(fill), p(words),
                                     0 if words is None else words.shape[1], 0 if words is None else words.shape[0], p(prd), p(exd[0]), p(exd[1]), k,
                                     p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), None)
    if expect:
        assert rc == expect, (rc, expect)
        return rc
    m.ctx.check(rc)
    return to_host(bufs)


def capped_want(U, lab, per, k, rows=None, pred="own", ex="own", bits=True, anchor=None):
    """The oracle on the poi_score_rows matrix for the same call -> ((ids, scores, labels, counts), bad rows)."""
    F = U.F
    rows = np.arange(U.n) if rows is None else np.asarray(rows)
    prd = F["pred"][rows] if isinstance(pred, str) else pred
    exl = sub_lists(F["ex"], rows) if isinstance(ex, str) else ex
    anc = F["anchor"][rows] if anchor is None else anchor
    pm = F["pmask"] if bits is True else np.ones((1, U.N), bool)
    mask, bad = FO.candidate_masks(pm, prd if bits is True else None, len(rows), exl[0], exl[1], anchor=anc)
    return CO.topk(U.score_rows()[rows], mask, lab, per, k), int(bad.sum())


@pytest.fixture(scope="module")
def fused(pa):
    cache = {}

    def get(kind, dim, seed=None):
        key = (kind, dim, seed)
        if key not in cache:
            cache[key] = Fused(pa, FC.fused_case(kind, dim, seed))
        return cache[key]
    return get


# ---- 3: the walk against the oracle on the poi_score_rows matrix ----------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", FC.FUSED_CASES)
def test_walk_is_the_oracle_on_the_score_rows(ctx, fused, kind, dim):
    U = fused(kind, dim)
    all_rows = np.arange(U.n)
    for name in ("three", "zipf", "mixed", "by id"):
        lab, n_label = CC.labeling(name, U.N)
        d_lab = dev(lab)
        fill = dev(CO.fill_table(lab, n_label, U.F["pmask"])[0])
        fill1 = dev(CO.fill_table(lab, n_label)[0])
        for per in (1, 2, 3):
            want, n_bad = capped_want(U, lab, per, 32)
            for k in CC.K_SET:
                assert_same(capped_call(U, d_lab, per, k, fill=fill), cut(want, k), "%s dim %d %s per %d k %d" % (kind, dim, name, per, k))
                assert ctx.take_bad_ids() == n_bad == 0
            for rows in (all_rows[:1], all_rows[20:53]):                             # n = 1, 33
                assert_same(capped_call(U, d_lab, per, 20, rows, fill=fill), cut(tuple(a[rows] for a in want), 20), "%s dim %d n %d" % (kind, dim, len(rows)))
            # bits NULL: every POI is a candidate, minus the lists; with the one-row fill table and without one
            want0, _ = capped_want(U, lab, per, FC.K, bits=None)
            assert_same(capped_call(U, d_lab, per, bits=None, fill=fill1), want0, "%s dim %d %s per %d bits NULL" % (kind, dim, name, per))
            assert_same(capped_call(U, d_lab, per, bits=None, pred=None), want0, "%s dim %d %s per %d bits NULL, fill NULL" % (kind, dim, name, per))
        # the sparse and the empty predicate for everyone; no lists
        for q in (FC.P_SPARSE, FC.P_NONE):
            want, _ = capped_want(U, lab, 1, FC.K, pred=np.full(U.n, q), ex=(None, None))
            got = capped_call(U, d_lab, 1, pred=np.full(U.n, q), ex=(None, None), fill=fill)
            assert_same(got, want, "%s dim %d %s predicate %d" % (kind, dim, name, q))
        assert (got[0] == -1).all() and (got[3] == 0).all()                          # nothing passes: nothing listed, count 0
    # where the cap cannot bind the existing entry is the yardstick: per = 32, and all labels distinct
    for k in (1, 20, 32):
        ref = U.call(WALK, k)
        for lab, per in ((CC.labeling("zipf", U.N)[0], 32), (CC.labeling("distinct", U.N)[0], 1), (np.full(U.N, -1, np.int32), 1)):
            got = capped_call(U, dev(lab), per, k)
            assert np.array_equal(got[0], ref[0]) and same_bits(got[1], ref[1]) and np.array_equal(got[3], ref[2]), (kind, dim, k, per)
            assert np.array_equal(got[2], np.where(got[0] >= 0, lab[np.maximum(got[0], 0)], -1))
    one = capped_call(U, dev(CC.labeling("one", U.N)[0]), 3, 20)                     # one label for every POI: the plain top-3
    assert np.array_equal(one[0][:, :3], ref[0][:, :3]) and (one[0][:, 3:] == -1).all()
    assert ctx.take_bad_ids() == 0


def test_walk_on_a_half_table(pa, ctx):
    import torch
    from tests import diverse_cases as DC
    H = DC.half_case()
    cat, flags = FC.attributes(DC.N_ITEM)
    pmask, _ = FO.pass_mask(cat, flags, FC.N_CAT, FC.PREDICATES)
    rng = np.random.default_rng(77)
    F = dict(pmask=pmask, pred=rng.integers(0, len(FC.PREDICATES), DC.N_USER), anchor=np.full(DC.N_USER, -1), ex=H["ex"], C=dict(T=dict(coords=H["coords"])))
    U = Fused(pa, F, build=H["build"])
    assert U.m.trained_items.t.dtype == torch.float16
    lab, n_label = CC.labeling("zipf", DC.N_ITEM)
    for per in (1, 2):
        want, _ = capped_want(U, lab, per, 32)
        assert_same(capped_call(U, dev(lab), per, 32), want, "half table per %d" % per)
    # the model path with exclude="train" against the oracle with the train lists
    m = U.m
    m.set_attributes(cat, flags, FC.N_CAT)
    filt = m.poi_filter(FC.PREDICATES)
    labels = pa.models.PoiLabels.from_categories(m, filt)
    assert np.array_equal(labels.fill.cpu().numpy(), CO.fill_table(cat, FC.N_CAT, pmask)[0])
    eo, ei = (t.cpu().numpy() for t in m.train_exclusion())
    rows = np.arange(DC.N_USER)
    got = m.compute_sub_topk_capped(rows, 20, labels, per=2, filt=filt, which=F["pred"], exclude="train", return_scores=True, return_labels=True,
                                    return_counts=True)
    want, _ = capped_want(U, cat, 2, 20, ex=(eo, ei))
    assert_same(tuple(t.cpu().numpy() for t in got), want, "half table, train lists")


# ---- 4, 5: planted tables whose float32 products are exact ------------------------------------------------------------------------------
def raw_call(ctx, users, items, lab, per, k, fill=None):
    """poi_score_topk_capped on plain tables: no distance term, no bitmap, no lists."""
    n, dim = users.shape
    bufs = out_buffers(n, k)
    ctx.check(ctx.lib.poi_score_topk_capped(ctx.handle, p(users), p(items), n, items.shape[0], dim, None, None, None, None, None, None, 0, 0.0, p(lab), per,
                                            p(fill), None, 0, 0, None, None, None, k, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), None))
    return to_host(bufs)


def test_planted_ties_through_the_product(ctx):
    users, items, sc = CC.tie_tables()
    d_users, d_items = dev(users), dev(items)
    mask = np.ones(sc.shape, bool)
    try:
        for name in ("three", "zipf", "mixed"):
            lab, n_label = CC.labeling(name, sc.shape[1])
            fill = dev(CO.fill_table(lab, n_label)[0])
            for per in (1, 2, 3):
                want = CO.topk(sc, mask, lab, per, 32)
                for split_max in (0, 256):
                    ctx.set_option("capped_split_max", split_max)
                    for k in (7, 20, 32):
                        assert_same(raw_call(ctx, d_users, d_items, dev(lab), per, k, fill), cut(want, k), "%s per %d k %d split_max %d" % (name, per, k, split_max))
    finally:
        ctx.set_option("capped_split_max", 256)


def test_the_merge_adversarially(ctx):
    """labels j % 64, k = 32, per = 1: row i is planted for GRIDS[i] slices - label L's best POI in slice L % S, a near-best POI of
    every label in every slice.  The best 64 of the slices' lists hold the first labels only; the pairwise merges must not care."""
    users, items, sc = CC.merge_tables()
    lab = CC.merge_labels()
    want = CO.topk(sc, np.ones(sc.shape, bool), lab, 1, 32)
    assert (want[2] == np.arange(32)[None]).all()
    d_users, d_items, d_lab = dev(users), dev(items), dev(lab)
    try:
        ctx.set_option("capped_split_max", 0)
        assert_same(raw_call(ctx, d_users, d_items, d_lab, 1, 32), want, "block regime")
        assert ctx.last_plan("capped_splits") == 0
        ctx.set_option("capped_split_max", BIG)
        for grid in CC.GRIDS + (0,):
            ctx.set_option("capped_grid", grid)
            assert_same(raw_call(ctx, d_users, d_items, d_lab, 1, 32), want, "grid %d" % grid)
            assert ctx.last_plan("capped_splits") == grid if grid else ctx.last_plan("capped_splits") >= 1
    finally:
        ctx.set_option("capped_split_max", 256); ctx.set_option("capped_grid", 0)


# ---- 6: grids, regimes, call sizes, the two entries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 32), ("spatial", 128)])
def test_every_grid_regime_and_call_size_gives_the_same_bits(ctx, fused, kind, dim):
    U = fused(kind, dim)
    lab, n_label = CC.labeling("zipf", U.N)
    d_lab, fill = dev(lab), dev(CO.fill_table(lab, n_label, U.F["pmask"])[0])
    try:
        for per in (1, 3):
            ctx.set_option("capped_split_max", 0); ctx.set_option("capped_grid", 0)
            base = capped_call(U, d_lab, per, 32, fill=fill)
            assert ctx.last_plan("capped_splits") == 0 and ctx.last_plan("capped_split_max") == 0
            for split_max, grid in ((256, 0), (BIG, 1), (BIG, 2), (BIG, 3), (BIG, 7), (BIG, 64)):
                ctx.set_option("capped_split_max", split_max); ctx.set_option("capped_grid", grid)
                assert_same(capped_call(U, d_lab, per, 32, fill=fill), base, "per %d split_max %d grid %d" % (per, split_max, grid))
                splits = ctx.last_plan("capped_splits")
                assert splits == grid if grid else splits >= 1
                assert ctx.last_plan("capped_split_max") == split_max
            ctx.set_option("capped_split_max", 256); ctx.set_option("capped_grid", 0)
            for r in (0, 31, 32, 69):                                                # a row alone against its place in the call of 70
                alone = capped_call(U, d_lab, per, 32, rows=[r], fill=fill)
                assert_same(alone, tuple(a[r:r + 1] for a in base), "row %d alone" % r)
            # the other entry on the matrix poi_score_rows writes
            F = U.F
            sc = dev(U.score_rows())
            got = capped_scores(ctx, sc, U.N, d_lab, per, 32, fill, U.words, dev(F["pred"].astype(np.int32)), dev_ex(F["ex"]))
            assert_same(got, base, "poi_topk_capped_scores on the score rows, per %d" % per)
    finally:
        ctx.set_option("capped_split_max", 256); ctx.set_option("capped_grid", 0)


# ---- 7: the fill gate ---------------------------------------------------------------------------------------------------------------------
def test_the_fill_gate_changes_no_bit(ctx, fused):
    U = fused("bpr", 64)
    lab, n_label = CC.labeling("three", U.N)
    d_lab = dev(lab)
    built = labels_build(ctx, lab, n_label)
    assert built[0][0, 2] == 6 and built[2] == 0
    over = dev(np.minimum(built[0] + 5, U.N))
    try:
        for split_max in (0, 256):
            ctx.set_option("capped_split_max", split_max)
            base = capped_call(U, d_lab, 2, 20, bits=None, pred=None, ex=(None, None), fill=built[3])
            assert ((base[0][:, :6] >= 0).all() and (base[0][:, 6:] == -1).all() and np.isneginf(base[1][:, 6:]).all() and (base[2][:, 6:] == -1).all())
            assert np.array_equal(np.sort(base[2][:, :6], axis=1), np.tile([0, 0, 1, 1, 2, 2], (U.n, 1))) and (base[3] == U.N).all()
            for fill in (None, over):
                assert_same(capped_call(U, d_lab, 2, 20, bits=None, pred=None, ex=(None, None), fill=fill), base, "fill %s" % ("NULL" if fill is None else "over"))
    finally:
        ctx.set_option("capped_split_max", 256)
    want, _ = capped_want(U, lab, 2, 20, bits=None, ex=(None, None))
    assert_same(base, want, "three labels, per 2")
    # a fill BELOW the true value is a caller error: the lists are cut there
    low = dev(np.full((1, 33), 4, np.int32))
    got = capped_call(U, d_lab, 2, 20, bits=None, pred=None, ex=(None, None), fill=low)
    assert np.array_equal(got[0][:, :4], base[0][:, :4]) and (got[0][:, 4:] == -1).all()


# ---- 8: independence from the project's own score rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", list(CC.ORACLE_SEEDS))
def test_both_entries_against_the_float64_oracle(ctx, fused, kind, dim):
    """Lists equal the float64 oracle's on the rows whose gaps are clear down to the depth the cap looks at (capped_oracle.qualifying);
    at least 90 % of the rows qualify - the seed was chosen so, under the oracle alone (tests/test_capped_cpu.py)."""
    U = fused(kind, dim, CC.ORACLE_SEEDS[(kind, dim)])
    F, osc, mask, lab = CC.oracle_case(kind, dim)
    d_lab = dev(lab)
    fill = dev(CO.fill_table(lab, 36, F["pmask"])[0])
    for per in CC.ORACLE_PERS:
        want = CO.topk(osc, mask, lab, per, FC.K)                    # (ranked on the float32-rounded oracle scores; the qualifying rows have no close calls)
        ok, depth = CO.qualifying(osc, mask, lab, per, FC.K)
        print("%s dim %d per %d: %.0f %% of %d rows qualify, depth up to %d" % (kind, dim, per, 100 * ok.mean(), len(ok), depth.max()))
        assert ok.mean() >= 0.9
        walk = capped_call(U, d_lab, per, fill=fill)
        rows = capped_scores(ctx, dev(osc.astype(np.float32)), U.N, d_lab, per, FC.K, fill, U.words, dev(F["pred"].astype(np.int32)), dev_ex(F["ex"]))
        for what, got in (("walk", walk), ("scores", rows)):
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[0][ok], want[0][ok]) and np.array_equal(got[2][ok], want[2][ok]), (what, per)
            live = got[0] >= 0
            err = np.abs(got[1][live] - np.take_along_axis(osc, np.maximum(got[0], 0), 1)[live]).max()
            print("  %s: max|score - oracle| = %.3g, bound %.3g" % (what, err, RTOL * np.abs(osc).max()))
            assert err <= RTOL * np.abs(osc).max()


# ---- 9: argument errors, bad rows --------------------------------------------------------------------------------------------------------
def test_argument_errors_and_bad_rows(ctx, fused):
    import torch
    U = fused("spatial", 32)
    lab, n_label = CC.labeling("zipf", U.N)
    d_lab = dev(lab)
    for k, per in ((0, 1), (33, 1), (20, 0), (20, 33)):
        assert capped_call(U, d_lab, per, k, expect=ENOTSUP) == ENOTSUP
    assert capped_call(U, d_lab, 1, dim=30, expect=ENOTSUP) == ENOTSUP
    assert capped_call(U, None, 1, expect=EINVAL) == EINVAL                          # NULL labels
    assert capped_call(U, d_lab, 1, bits=U.words[:, :-3].contiguous(), expect=EINVAL) == EINVAL      # ldw < W
    got = capped_call(U, d_lab, 1, rows=[0], n_arg=0)                                # n = 0: a no-op
    assert (got[0] == -7).all() and (got[1] == 7.0).all() and (got[2] == -7).all() and (got[3] == -7).all()
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    zf = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    for k, per, ldw, labels, want in ((0, 1, 2, z, ENOTSUP), (33, 1, 2, z, ENOTSUP), (5, 0, 2, z, ENOTSUP), (5, 33, 2, z, ENOTSUP), (5, 1, 1, z, EINVAL),
                                      (5, 1, 2, None, EINVAL)):
        assert ctx.lib.poi_topk_capped_scores(ctx.handle, p(zf), 2, 64, 64, p(labels), per, None, p(z), ldw, 1, None, None, None, k, p(z), None, None, None,
                                              None) == want, (k, per, ldw)
    assert ctx.lib.poi_topk_capped_scores(ctx.handle, p(zf), 0, 64, 64, p(z), 1, None, None, 0, 0, None, None, None, 5, p(z), None, None, None, None) == 0
    assert (z == 0).all() and ctx.take_bad_ids() == 0
    # device-side bad rows, in both regimes: predicate index, anchor, a descending list, a list that leaves the table
    F = U.F
    pred, anchor = F["pred"].copy(), F["anchor"].copy()
    pred[7], pred[33] = len(FC.PREDICATES), -1
    anchor[9], anchor[41] = U.N, -2
    lists = [F["ex"][1][F["ex"][0][r]:F["ex"][0][r + 1]] for r in range(U.n)]
    lists[11], lists[50] = np.array([5, 5]), np.array([0, U.N])
    ex = FO.csr(lists)
    want, n_bad = capped_want(U, lab, 2, FC.K, pred=pred, ex=ex, anchor=anchor)
    assert n_bad == 6 and (want[3][[7, 33, 9, 41, 11, 50]] == 0).all()
    fill = dev(CO.fill_table(lab, n_label, F["pmask"])[0])
    try:
        for split_max in (256, 0):
            ctx.set_option("capped_split_max", split_max)
            got = capped_call(U, d_lab, 2, pred=pred, ex=ex, anchor=dev(anchor.astype(np.int32)), fill=fill)
            assert_same(got, want, "bad rows, split_max %d" % split_max)
            assert ctx.take_bad_ids() == 6                                           # each counted once, whatever the slices
    finally:
        ctx.set_option("capped_split_max", 256)


# ---- 10: Python --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bpr", 32), ("spatial", 64)])
def test_model_call_against_the_oracle(pa, ctx, fused, kind, dim):
    import torch
    from poi_amd import evaluate as E
    U = fused(kind, dim, CC.ORACLE_SEEDS[(kind, dim)])
    m, F = U.m, U.F
    rows = np.arange(U.n)
    full = m.compute_sub_all_scores_device(rows).cpu().numpy()
    m.set_attributes(F["cat"], F["flags"], FC.N_CAT)
    filt = m.poi_filter(FC.PREDICATES)
    for f, pm in ((None, None), (filt, F["pmask"])):
        labels = pa.models.PoiLabels.from_categories(m, f)
        want_fill, want_cnt, _ = CO.fill_table(F["cat"], FC.N_CAT, pm)
        assert np.array_equal(labels.fill.cpu().numpy(), want_fill) and np.array_equal(labels.counts, want_cnt) and labels.n_label == FC.N_CAT
        which = None if f is None else F["pred"]
        mask, _ = FO.candidate_masks(np.ones((1, U.N), bool) if pm is None else pm, which, U.n, *F["ex"])
        for per in (1, 2):
            got = m.compute_sub_topk_capped(rows, FC.K, labels, per=per, filt=f, which=which, exclude=F["ex"], return_scores=True, return_labels=True,
                                            return_counts=True)
            want = CO.topk(full, mask, F["cat"], per, FC.K)
            got = tuple(t.cpu().numpy() for t in got)
            # (compute_sub_all_scores_device sums in another order than the walk: ids on the rows the oracle qualifies, scores to RTOL)
            ok, _ = CO.qualifying(full.astype(np.float64), mask, F["cat"], per, FC.K)
            assert ok.mean() >= 0.9 and np.array_equal(got[0][ok], want[0][ok]) and np.array_equal(got[3], want[3]), (kind, per)
            live = ok[:, None] & (got[0] >= 0)
            assert np.abs(got[1][live] - want[1][live]).max() <= RTOL * np.abs(full).max()
            assert np.array_equal(got[2], np.where(got[0] >= 0, F["cat"][np.maximum(got[0], 0)], -1))
        if f is None:
            distinct, share = E.label_spread(got[0], F["cat"])                       # (per = 2 lists)
            assert (share <= 2 / (got[0] >= 0).sum(axis=1) + 1e-12).all()
            one = m.compute_sub_topk_capped(rows, FC.K, labels, per=1)
            d1, s1 = E.label_spread(one, F["cat"])
            assert np.array_equal(d1, (one.cpu().numpy() >= 0).sum(axis=1)) and np.allclose(s1, 1.0 / d1)
            # exclude="train", a plain label array, labels built for another filter (the gate falls back to k): the same lists
            a = m.compute_sub_topk_capped(rows, FC.K, labels, per=2, exclude="train")
            b = m.compute_sub_topk_capped(rows, FC.K, F["cat"], per=2, exclude=tuple(t for t in m.train_exclusion()))
            assert torch.equal(a, b)
    c = m.compute_sub_topk_capped(rows, FC.K, labels, per=2, exclude="train")      # labels built with filt, the call without: fill NULL
    assert torch.equal(a, c)
    with pytest.raises(ValueError):
        m.compute_sub_topk_capped(rows, 33, labels)
    with pytest.raises(ValueError):
        m.compute_sub_topk_capped(rows, 5, labels, per=0)
    with pytest.raises(ValueError):
        m.compute_sub_topk_capped(rows, 5, labels, which=F["pred"])                  # which without filt
    with pytest.raises(IndexError):
        m.compute_sub_topk_capped(rows, 5, labels, filt=filt, which=np.full(U.n, len(FC.PREDICATES)))
    with pytest.raises(ValueError):
        m.poi_labels(F["cat"][:-1])
    with pytest.raises(IndexError, match="POI"):
        m.poi_labels(F["cat"], n_label=20)
    with pytest.raises(IndexError, match="1 row"):
        m.compute_sub_topk_capped(rows, 5, labels, filt=filt, which=dev(np.r_[np.zeros(U.n - 1), [99]].astype(np.int32)))
    out = m.compute_sub_topk_capped(rows, 5, labels, filt=filt, which=dev(np.r_[np.zeros(U.n - 1), [99]].astype(np.int32)), sync=False)
    assert (out[-1] == -1).all() and ctx.take_bad_ids() == 1


def fused_model(pa, cls):
    """One small model of a class that scores by users . items, beside OboBpr and OboSpatialGru above: (model, users)."""
    from poi_amd import data as D
    if cls in ("gru", "vbpr", "fpmc"):                   # OboGru, OboVBpr (kdim = 2 D, items [lt | fi ei^T]), OboFpmc_lr (kdim = 2 D)
        from tests.test_gpu_audience import rank_model
        return rank_model(pa, cls, 20, 70)[0], np.arange(70)
    if cls == "geoie":                                   # OboGeoIE under its default rule: _rank_fused is a property
        from tests.test_gpu_geoie import _model as geoie_model
        ds = D.make_synthetic(24, 50, 10, 5)
        m = geoie_model(ds, dim=8, d_min=0.01)
        m.train_batch(np.arange(ds.n_user))
        m.update_trained()
        return m, np.arange(24)
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC      # Lstm / Rnn: the model call, not a session
    T = TS.geo_problem(61, n_user=40, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    m = TC.model(pa, cls, T, TC.params(cls, 61, T))
    m.update_trained_users(m.predict_device(np.arange(T["n_user"])))
    return m, np.arange(T["n_user"])


@pytest.mark.parametrize("cls", ["gru", "vbpr", "fpmc", "geoie", "lstm", "rnn"])
def test_every_other_fused_class_against_the_oracle_on_its_own_score_rows(pa, ctx, cls):
    """compute_sub_topk_capped against the oracle on the model's own compute_sub_all_scores_device rows.  Those rows are summed in
    another order than the walk's product, so the ids are held on the rows the oracle qualifies (at least 90 %), the scores to RTOL;
    counts and labels on every row."""
    m, users = fused_model(pa, cls)
    assert m._rank_fused, cls
    n, N = len(users), m.n_item
    full = m.compute_sub_all_scores_device(users).cpu().numpy()
    assert full.shape == (n, N)
    lab = (np.arange(N) * 7 % 6).astype(np.int32)
    lab[::9] = -1
    labels = m.poi_labels(lab)
    assert np.array_equal(labels.fill.cpu().numpy(), CO.fill_table(lab, 6)[0])
    lists = FO.csr([np.sort(np.random.default_rng(r).choice(N, r % 20, replace=False)) for r in range(n)])
    mask, _ = FO.candidate_masks(np.ones((1, N), bool), None, n, *lists)
    for per in (1, 2):
        got = m.compute_sub_topk_capped(users, 10, labels, per=per, exclude=lists, return_scores=True, return_labels=True, return_counts=True)
        got = tuple(t.cpu().numpy() for t in got)
        want = CO.topk(full, mask, lab, per, 10)
        ok, _ = CO.qualifying(full.astype(np.float64), mask, lab, per, 10)
        print("%s per %d: %.0f %% of %d rows qualify" % (cls, per, 100 * ok.mean(), n))
        assert ok.mean() >= 0.9 and np.array_equal(got[0][ok], want[0][ok]) and np.array_equal(got[3], want[3]), (cls, per)
        live = ok[:, None] & (got[0] >= 0)
        assert np.abs(got[1][live] - want[1][live]).max() <= RTOL * np.abs(full).max()
        assert np.array_equal(got[2], np.where(got[0] >= 0, lab[np.maximum(got[0], 0)], -1))
    assert ctx.take_bad_ids() == 0


def own_rule_models(pa):
    """(name, model, users): one small model of each of the four classes that rank by a rule of their own - with
    test_model_call_against_the_oracle (OboBpr, OboSpatialGru) and fused_model, every model class."""
    from poi_amd import data as D
    from tests.test_gpu_group import carnn_model
    from tests.test_gpu_prme import _model as prme_model
    from tests.test_gpu_geoie import _model as geoie_model
    from tests.test_gpu_poi2vec import model_of, problem
    yield "carnn", carnn_model(pa), np.arange(21)
    ds = D.make_prme_synthetic(24, 50, 10, 4)
    m = prme_model(ds, dim=8)
    m.update_trained_items()
    yield "prme", m, np.arange(24)
    rng = np.random.default_rng(19)
    pr = problem(300, 50, 8, [int(x) for x in rng.integers(3, 9, 24)])
    m = model_of(pr, softmax_axis="items", eval_context="test")
    m.update_trained_params()
    yield "poi2vec", m, np.arange(24)
    ds = D.make_synthetic(24, 50, 10, 5)
    m = geoie_model(ds, dim=8, d_min=0.01)
    m.train_batch(np.arange(ds.n_user))
    m.update_trained()
    m.score_rule = "geo"
    yield "geoie", m, np.arange(24)


def test_own_rule_models_go_through_their_own_score_rows(pa, ctx):
    for name, m, users in own_rule_models(pa):
        assert not m._rank_fused, name
        n, N = len(users), m.n_item
        full = m._own_score_rows(users)(0, n).cpu().numpy()                          # the model's score rows, position 0 of every user
        if name in ("carnn", "geoie"):                                               # (PRME and POI2Vec rank (user, position) rows: position 0)
            ref = m.compute_sub_all_scores_device(users).cpu().numpy()
            assert np.array_equal(full.view(np.uint32), ref.view(np.uint32)), name
        lab = (np.arange(N) * 7 % 5).astype(np.int32)
        lab[::9] = -1
        labels = m.poi_labels(lab)
        lists = FO.csr([np.sort(np.random.default_rng(r).choice(N, r % 20, replace=False)) for r in range(n)])
        mask, _ = FO.candidate_masks(np.ones((1, N), bool), None, n, *lists)
        for per in (1, 2):
            got = m.compute_sub_topk_capped(users, 10, labels, per=per, exclude=lists, return_scores=True, return_labels=True, return_counts=True)
            assert_same(tuple(t.cpu().numpy() for t in got), CO.topk(full, mask, lab, per, 10), "%s per %d" % (name, per))


@pytest.mark.parametrize("kind", ["spatial", "lstm", "carnn"])
def test_session_recommend_capped_is_the_oracle_on_the_sessions_scores(pa, kind):
    import torch
    from tests import test_gpu_session as TS, test_gpu_session_cells as TC
    T = TS.geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    if kind == "spatial":
        m = TS.spatial_model(pa, T, TS.spatial_init(32, T))
        s = m.session(n_slot=T["n_user"])
    else:
        m = TC.model(pa, kind, T, TC.params(kind, 60, T))
        if kind == "lstm":
            m.set_coords(T["coords"])
        s = m.cell_session(n_slot=T["n_user"])
    slots = np.arange(T["n_user"])
    for t in range(3):
        s.advance(slots[:-2], T["train"][0][:-2, t])     # the last two slots never check in
    lab = CC.labeling("zipf", 1003)[0][:300].copy()
    lab[::11] = -1
    labels = m.poi_labels(lab)
    lists = FO.csr([np.sort(np.random.default_rng(r).choice(300, r % 40, replace=False)) for r in range(T["n_user"])])
    mask, _ = FO.candidate_masks(np.ones((1, 300), bool), None, T["n_user"], *lists)
    # the session's own scores of every POI, in the order of its own ranking: candidates(k = n_item) returns ids and score bits
    if kind == "carnn":
        n, score_rows, has, _ = s._carnn_rows(slots)
        full = score_rows(0, n).cpu().numpy()
        full[~has.cpu().numpy()] = -np.inf
    else:
        ids, sc = (t.cpu().numpy() for t in s.candidates(slots, 300, return_scores=True))
        full = np.full((T["n_user"], 300), -np.inf, np.float32)
        np.put_along_axis(full, ids, sc, 1)
    for per in (1, 2):
        got = s.recommend_capped(slots, 20, labels, per=per, exclude=dev_ex(lists), return_scores=True, return_labels=True, return_counts=True)
        got = tuple(t.cpu().numpy() for t in got)
        want = CO.topk(full, mask, lab, per, 20)
        if kind == "carnn":                              # a slot without a check-in: nothing ranked, count 0
            want[3][-2:] = 0
        assert_same(got, want, "%s session per %d" % (kind, per))
    if kind != "carnn":
        last = s.recommend_capped(slots[:5], 20, labels, exclude="last", return_counts=True)
        assert np.all(last[1].cpu().numpy() == 299)
    with pytest.raises(ValueError):
        s.recommend_capped(slots, 20, labels, exclude="train")
    with pytest.raises(ValueError):
        s.recommend_capped(slots, 33, labels)
