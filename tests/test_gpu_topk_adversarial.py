"""-m gpu: the streaming top-K (score_topk.hip, with score_filter.hip in front of it) on PLANTED score rows - tests/topk_streams.py -
against oracle.poi_oracle.topk_desc on the same matrix, ids and score bits with zero tolerance, no row masked out.

Random scores never tie and let every threshold settle within two tiles; these rows hold exact ties at every rank, a plateau at the
cut that spans item ranges, constant rows, staircases that keep the candidate lists at 65 .. 80 entries (the second readlane loop of
compact_user, its upper-half K-th best, slot 79), winners in the first / last items of a ragged table and values that only differ below
half precision.  Two ways carry an arbitrary row S into the kernels exactly:
  prob path      users = 0, wd = 1, prob = S: score = fma(1, S, 0) = S                       (poi_score_topk: variant 0, packed, dim 256)
  one-hot path   users[u] = e_(u mod D), items[j][c] = S[c][j]: score = S[u mod D], plus a distance term wd * sts[bin] with wd = 2 and
                 sts in multiples of 2^-6 (exact)                                            (two-stage filter, bin matrix, GEO)
N = 2048 + 17 = 65 item tiles: eight ranges of nine tiles at these user counts (abi.hip, splits_for); N = 8192 + 17 = 257 tiles lets an
unseeded call take the self-seeding passes of the two-stage path."""
import functools
import time

import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import topk_streams as TS

pytestmark = pytest.mark.gpu

KS = (1, 5, 20, 31, 32)
N0 = 2048 + 17
N1 = 8192 + 17
WD = 2.0
COORDS4 = np.array([[40.0, -74.0], [40.01, -74.0], [40.0, -73.98], [40.5, -73.5]])       # 0 m, 1.1 km, 1.7 km, ~70 km apart: bins 0 / 5 / 8 / too far (> 300 bins of 200 m)


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _families(N, K, with_g=False):
    names, S = TS.family_rows(N, K, with_g)
    assert TS.is_exact(S)
    return names, S


@functools.lru_cache(maxsize=None)
def _expected(N, K, with_g=False):
    names, S = _families(N, K, with_g)
    return TS.expected_lists(S, K, O.topk_desc)


def _assert_lists(got, exp, label, names=None, cls=None):
    (idx, sc), (eidx, esc) = got, exp
    assert idx.shape == eidx.shape and sc.shape == esc.shape, (label, idx.shape, eidx.shape)
    bad = np.flatnonzero((idx != eidx).any(axis=1) | (sc.view(np.uint32) != esc.view(np.uint32)).any(axis=1))
    if bad.size:
        r = int(bad[0])
        fam = names[cls[r]] if names is not None and cls is not None and cls[r] < len(names) else "-"
        raise AssertionError("%s: %d of %d rows differ from the oracle; first: row %d (family %s)\n got ids %s\n exp ids %s\n got sc %s\n exp sc %s"
                             % (label, bad.size, idx.shape[0], r, fam, idx[r].tolist(), eidx[r].tolist(), sc[r].tolist(), esc[r].tolist()))


def _run(ctx, call, n, K, seed=None, filt=None):
    import torch
    idx = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    sc = torch.zeros((n, K), dtype=torch.float32, device="cuda")
    try:
        if filt is not None:
            ctx.set_topk_filter(filt)
        if seed is not None:
            ctx.set_topk_seed(seed, seed.shape[1])
        ctx.check(call(idx, sc))
        return idx.cpu().numpy(), sc.cpu().numpy()
    finally:
        ctx.set_topk_filter(True)


def _seeds(S_rows, eidx, rng):
    """Per row of S_rows: the true list; the true list with every tied member replaced by the HIGHEST-index non-members of the same
    score (as many as exist); a random list of distinct ids."""
    n, K = eidx.shape
    N = S_rows.shape[1]
    swapped = eidx.copy()
    for r in range(n):
        row, lst = S_rows[r], eidx[r]
        for v in np.unique(row[lst]):
            pos = np.flatnonzero(row[lst] == v)
            pool = np.setdiff1d(np.flatnonzero(row == v), lst)
            take = min(len(pos), len(pool))
            if take:
                swapped[r, pos[len(pos) - take:]] = pool[len(pool) - take:]
    rnd = np.stack([rng.choice(N, K, replace=False) for _ in range(n)])
    return [("true list", eidx.astype(np.int32)), ("ties swapped for higher ids", swapped.astype(np.int32)), ("random list", rnd.astype(np.int32))]


# ---- prob path --------------------------------------------------------------------------------------------------------------------------
def _prob_problem(n, dim, N, K):
    names, S = _families(N, K)
    cls = np.arange(n) % len(names)
    rng = np.random.default_rng(n + dim)
    users = np.zeros((n, dim), np.float32)
    items = rng.standard_normal((N, dim)).astype(np.float32)          # multiplied by zero
    eidx, esc = _expected(N, K)
    return names, S, cls, users, items, S[cls].astype(np.float32), (eidx[cls], esc[cls])


def _prob_call(ctx, du, di, dwd, dp, n, N, dim, K):
    return lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, dwd.data_ptr(), dp.data_ptr(), K, idx.data_ptr(), sc.data_ptr(), None)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n,dim", [(33, 32), (160, 32), (160, 256)])
def test_score_topk_prob_path_every_family(pa, n, dim, K):
    """Variant 0 (row-per-lane, n < 128), the packed-stream variant, and variant 0 at dim 256 - unseeded, then seeded with the true
    list, with a list whose tied members are OTHER members of the same plateau, and with a random list."""
    ctx = pa._lib.context(0)
    names, S, cls, users, items, prob, exp = _prob_problem(n, dim, N0, K)
    du, di, dp, dwd = _dev(users), _dev(items), _dev(prob), _dev(np.array([1.0], np.float32))
    call = _prob_call(ctx, du, di, dwd, dp, n, N0, dim, K)
    _assert_lists(_run(ctx, call, n, K), exp, "unseeded", names, cls)
    for what, seed in _seeds(S[cls], exp[0], np.random.default_rng(K)):
        _assert_lists(_run(ctx, call, n, K, seed=_dev(seed)), exp, "seeded: " + what, names, cls)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", [1, 31, 32])
def test_score_topk_prob_path_small_tables(pa, n, K):
    """Tables of one or two (ragged) item tiles, down to N = K: four item ranges of which some are empty."""
    ctx = pa._lib.context(0)
    for N in sorted({K, 32, 33, 64, 65, 95}):                     # (95: a 31-item tail with K < N - the winners of family f sit in it)
        if N < K:
            continue
        names, S, cls, users, items, prob, exp = _prob_problem(n, 32, N, K)
        du, di, dp, dwd = _dev(users), _dev(items), _dev(prob), _dev(np.array([1.0], np.float32))
        _assert_lists(_run(ctx, _prob_call(ctx, du, di, dwd, dp, n, N, 32, K), n, K), exp, "N = %d" % N, names, cls)


# ---- one-hot path -----------------------------------------------------------------------------------------------------------------------
def _geo_tables(n, dim, N, n_dist, seed):
    """Distance term of the one-hot path: every item sits on one of four points, the last POI and the bin-probability row of a user
    depend on the class of the user only - `dim` distinct score rows.  Returns the device-side arrays and term (dim, N) float64 = wd * sts[bin]."""
    from poi_amd.data import cal_dis_vec
    rng = np.random.default_rng(seed)
    dd = 200.0
    coords = COORDS4[np.arange(N) % 4]
    last_c = (np.arange(dim) * 5 + 1) % N                                                # class -> last POI
    tab = rng.integers(0, 64, (8, n_dist + 1)) / 64.0
    tab[:, n_dist] = 0.0
    tab[3] = 0.0                                                                         # (classes 3 mod 8: no distance term at all)
    term = np.zeros((dim, N))
    for c in range(dim):
        b = cal_dis_vec(coords[last_c[c], 0], coords[last_c[c], 1], coords[:, 0], coords[:, 1], dd, n_dist)
        term[c] = WD * np.where(b < n_dist, tab[c % 8][np.minimum(b, n_dist)], 0.0)
    cls = np.arange(n) % dim
    npad = ((n + 31) // 32) * 32
    sts = np.zeros((npad, n_dist + 1), np.float32)
    sts[:n] = tab[cls % 8]
    return dict(coords=coords, last=last_c[cls].astype(np.int32), sts=sts, dd=dd, n_dist=n_dist), term


def _one_hot_problem(n, dim, N, K, with_g=False, n_dist=0, seed=0):
    names, S = _families(N, K, with_g)
    users, items, full = TS.one_hot(S, n, dim)
    geo = None
    if n_dist:
        geo, term = _geo_tables(n, dim, N, n_dist, seed)
        full = full + term
        assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    cls = np.arange(n) % dim
    eidx, esc = TS.expected_lists(full, K, O.topk_desc)
    return names, full, cls, users, items, geo, (eidx[cls], esc[cls])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dim", [64, 128])
def test_score_topk_one_hot_filter_paths(pa, dim, K):
    """257 item tiles: the unseeded two-stage call seeds itself (block maxima of the f16 pass), the filter keeps what can beat the bound
    and the survivors are rescored exactly; constant rows overflow the survivor lists and fall back to the one-stage kernel with the
    same bounds.  One-stage, two-stage and two-stage seeded with the true list - each against the oracle.  NOTE: with constant rows, zero
    padding classes and the dense family g in every 32-user tile, EVERY tile overflows here: this pins the overflow fallback (the one-stage
    kernel started from the filter's bounds), not the rescore kernel - that is test_score_topk_two_stage_lists_come_from_the_rescore_kernel."""
    ctx = pa._lib.context(0)
    n = 160
    names, full, cls, users, items, _, exp = _one_hot_problem(n, dim, N1, K, with_g=True)
    du, di = _dev(users), _dev(items)
    call = lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N1, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
    _assert_lists(_run(ctx, call, n, K, filt=False), exp, "one-stage", names, cls)
    _assert_lists(_run(ctx, call, n, K, filt=True), exp, "two-stage, self-seeded", names, cls)
    _assert_lists(_run(ctx, call, n, K, seed=_dev(exp[0]), filt=True), exp, "two-stage, seeded with the true list", names, cls)


def _rescored(ctx, call, n, K, seed=None):
    """A two-stage call whose lists really come from score_rescore_kernel: the kernel ran in THIS call (timing: one launch) and no
    user tile overflowed its survivor lists (a flagged tile is redone by the one-stage kernel and would hide the filter's result)."""
    ctx.timing(True)
    try:
        got = _run(ctx, call, n, K, seed=seed, filt=True)
        launches = ctx.timing_get("score_rescore")[1]
    finally:
        ctx.timing(False)
    st = ctx.topk_filter_stats()
    assert launches == 1, "the call did not take the two-stage path"
    assert st["users"] == n and st["tiles"] == (n + 31) // 32 and st["tiles_flagged"] == 0, st
    assert st["survivors"] >= n * K, st                      # (every list member is a survivor)
    return got


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dim", [64, 128])
def test_score_topk_two_stage_lists_come_from_the_rescore_kernel(pa, dim, K):
    """The f16 survivor rule on exact ties and the rescore kernel's K-best selection over long tied survivor lists, on rows that cannot
    overflow (topk_streams.filter_rows; sparse g: values that differ only below half precision): every tile's result is the two-stage
    path's own - asserted from the call's statistics.  65 tiles seeded (true list, ties swapped for higher ids); 257 tiles self-seeded
    from the block maxima, and seeded."""
    ctx = pa._lib.context(0)
    n = 160
    for N in (N0, N1):
        names, S = TS.filter_rows(N, K)
        users, items, full = TS.one_hot(S, n, dim, n_cls=len(names))
        cls = np.arange(n) % len(names)
        eidx, esc = TS.expected_lists(S, K, O.topk_desc)
        exp = (eidx[cls], esc[cls])
        du, di = _dev(users), _dev(items)
        call = lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
        _assert_lists(_run(ctx, call, n, K, filt=False), exp, "N = %d, one-stage" % N, names, cls)
        for what, seed in _seeds(S[cls], exp[0], np.random.default_rng(K))[:2]:
            _assert_lists(_rescored(ctx, call, n, K, seed=_dev(seed)), exp, "N = %d, two-stage seeded: %s" % (N, what), names, cls)
        if N == N1:
            _assert_lists(_rescored(ctx, call, n, K), exp, "N = %d, two-stage self-seeded" % N, names, cls)


@pytest.mark.parametrize("K", [5, 32])
def test_nan_items_never_enter_the_two_stage_lists(pa, K):
    """Every sixteenth item row is NaN: its score is NaN for every user.  A NaN survives the filter by design; the rescore kernel must drop
    it as the one-stage kernels do (`score > threshold` is false) - seeded with the true list at 65 tiles, self-seeded at 257."""
    ctx = pa._lib.context(0)
    n, dim = 160, 64
    for N in (N0, N1):
        names, S = TS.filter_rows(N, K)
        users, items, full = TS.one_hot(S, n, dim, n_cls=len(names))
        items[5::16] = np.nan
        full[:, 5::16] = np.nan
        cls = np.arange(n) % len(names)
        eidx, esc = TS.expected_lists(full[:len(names)], K, O.topk_desc)
        exp = (eidx[cls], esc[cls])
        assert (exp[0] >= 0).all() and (exp[0] % 16 != 5).all()
        du, di = _dev(users), _dev(items)
        call = lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
        _assert_lists(_run(ctx, call, n, K, filt=False), exp, "N = %d, one-stage" % N, names, cls)
        _assert_lists(_rescored(ctx, call, n, K, seed=_dev(exp[0])), exp, "N = %d, two-stage seeded with the true list" % N, names, cls)
        if N == N1:
            _assert_lists(_rescored(ctx, call, n, K), exp, "N = %d, two-stage self-seeded" % N, names, cls)


@pytest.mark.parametrize("K", [5, 32])
@pytest.mark.parametrize("entry", ["geo", "ulptai"])
def test_short_rows_on_the_bin_paths(pa, entry, K):
    """poi_score_topk_geo / _ulptai: all item rows but three are NaN, and the users of class 5 mod 8 have -inf in every bin of their
    probability row (items in reach score -inf, items too far away keep the plain score): never selected, -1 / -inf tail."""
    import torch
    from poi_amd.data import bin_thresholds, cos_lat
    ctx = pa._lib.context(0)
    n, dim, N, n_dist = 160, 64, N0, 200
    names, S = _families(N, K)
    users, items, full = TS.one_hot(S, n, dim)
    keep = [0, N // 2, N - 1]
    g, term = _geo_tables(n, dim, N, n_dist, 7)
    with np.errstate(invalid="ignore"):
        term[5::8] = np.where(term[5::8] != 0.0, -np.inf, term[5::8])            # (bins in reach with a zero probability stay zero)
    g["sts"][:n][(np.arange(n) % dim) % 8 == 5] = np.where(g["sts"][:n][(np.arange(n) % dim) % 8 == 5] != 0.0, -np.inf, 0.0)
    full = full + term
    nan = np.ones(N, bool); nan[keep] = False
    items[nan] = np.nan
    full[:, nan] = np.nan
    cls = np.arange(n) % dim
    eidx, esc = TS.expected_lists(full, K, O.topk_desc)
    exp = (eidx[cls], esc[cls])
    assert (exp[0][:, 3:] == -1).all()
    du, di, dwd, dsts = _dev(users), _dev(items), _dev(np.array([WD], np.float32)), _dev(g["sts"])
    dc, cph, thr, dl = _dev(g["coords"]), _dev(cos_lat(g["coords"])), _dev(bin_thresholds(g["dd"], n_dist)), _dev(g["last"])
    if entry == "geo":
        call = lambda idx, sc: ctx.lib.poi_score_topk_geo(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, dwd.data_ptr(), dsts.data_ptr(), dc.data_ptr(), cph.data_ptr(),
                                                          thr.data_ptr(), dl.data_ptr(), n_dist, g["dd"], K, idx.data_ptr(), sc.data_ptr(), None)
    else:
        bins = torch.zeros(((n + 31) // 32) * ((N + 31) // 32) * 1024, dtype=torch.uint8, device="cuda")
        ctx.check(ctx.lib.poi_ulptai_build(ctx.handle, dc.data_ptr(), cph.data_ptr(), thr.data_ptr(), dl.data_ptr(), n, N, n_dist, g["dd"], bins.data_ptr(), 1, None))
        call = lambda idx, sc: ctx.lib.poi_score_topk_ulptai(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, dwd.data_ptr(), dsts.data_ptr(), bins.data_ptr(), 1, n_dist, K,
                                                             idx.data_ptr(), sc.data_ptr(), None)
    _assert_lists(_run(ctx, call, n, K, filt=False), exp, "one-stage")
    _assert_lists(_run(ctx, call, n, K, filt=True), exp, "default path")
    rnd = np.stack([np.random.default_rng(u).choice(N, K, replace=False) for u in range(n)]).astype(np.int32)
    _assert_lists(_run(ctx, call, n, K, seed=_dev(rnd), filt=True), exp, "seeded with random ids (NaN / -inf bounds)")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_dist", [200, 300])
def test_score_topk_ulptai_planted_bins(pa, n_dist, K):
    """Resident bin matrix, uint8 (200 bins) and uint16 (300): all items on four points, so (dot, bin) pairs tie in bulk."""
    import torch
    from poi_amd.data import bin_thresholds, cos_lat
    ctx = pa._lib.context(0)
    n, dim, N = 160, 64, N0
    names, full, cls, users, items, g, exp = _one_hot_problem(n, dim, N, K, n_dist=n_dist, seed=n_dist)
    bb = 1 if n_dist <= 255 else 2
    du, di, dwd, dsts = _dev(users), _dev(items), _dev(np.array([WD], np.float32)), _dev(g["sts"])
    dc, cph, thr, dl = _dev(g["coords"]), _dev(cos_lat(g["coords"])), _dev(bin_thresholds(g["dd"], n_dist)), _dev(g["last"])
    bins = torch.zeros(((n + 31) // 32) * ((N + 31) // 32) * 1024 * bb, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.poi_ulptai_build(ctx.handle, dc.data_ptr(), cph.data_ptr(), thr.data_ptr(), dl.data_ptr(), n, N, n_dist, g["dd"], bins.data_ptr(), bb, None))
    call = lambda idx, sc: ctx.lib.poi_score_topk_ulptai(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, dwd.data_ptr(), dsts.data_ptr(), bins.data_ptr(), bb, n_dist, K,
                                                         idx.data_ptr(), sc.data_ptr(), None)
    _assert_lists(_run(ctx, call, n, K, filt=False), exp, "one-stage", names, cls)
    _assert_lists(_run(ctx, call, n, K, filt=True), exp, "default path, unseeded", names, cls)
    _assert_lists(_run(ctx, call, n, K, seed=_dev(exp[0]), filt=True), exp, "two-stage, seeded with the true list", names, cls)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dim,n,N,modes", [(64, 160, N0, (True,)), (128, 1024, N0, (True,)), (256, 1024, N0, ("items", "users")), (64, 160, N1, (True,))])
def test_score_topk_geo_planted(pa, dim, n, N, modes, K):
    """Bins on the fly: the row-per-lane kernel, the packed-stream kernel (n >= 1024, dim >= 128) at dims 128 and 256, each one-stage
    unseeded and two-stage seeded with the true list (dim 256: item- and user-stationary filter).  The 257-tile table adds the unseeded
    two-stage call, whose bounds come from the one-stage kernel on a prefix of the table."""
    from poi_amd.data import bin_thresholds, cos_lat
    ctx = pa._lib.context(0)
    n_dist = 200
    names, full, cls, users, items, g, exp = _one_hot_problem(n, dim, N, K, n_dist=n_dist, seed=dim)
    du, di, dwd, dsts = _dev(users), _dev(items), _dev(np.array([WD], np.float32)), _dev(g["sts"])
    dc, cph, thr, dl = _dev(g["coords"]), _dev(cos_lat(g["coords"])), _dev(bin_thresholds(g["dd"], n_dist)), _dev(g["last"])
    call = lambda idx, sc: ctx.lib.poi_score_topk_geo(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, dwd.data_ptr(), dsts.data_ptr(), dc.data_ptr(), cph.data_ptr(),
                                                      thr.data_ptr(), dl.data_ptr(), n_dist, g["dd"], K, idx.data_ptr(), sc.data_ptr(), None)
    _assert_lists(_run(ctx, call, n, K, filt=False), exp, "one-stage", names, cls)
    for mode in modes:
        _assert_lists(_run(ctx, call, n, K, seed=_dev(exp[0]), filt=mode), exp, "two-stage (%s), seeded with the true list" % mode, names, cls)
        if N == N1:
            _assert_lists(_run(ctx, call, n, K, filt=mode), exp, "two-stage (%s), self-seeded from a prefix" % mode, names, cls)


# ---- explicit rows ----------------------------------------------------------------------------------------------------------------------
def _topk_rows(ctx, S32, K):
    d = _dev(S32)
    n, N = S32.shape
    return _run(ctx, lambda idx, sc: ctx.lib.poi_topk(ctx.handle, d.data_ptr(), n, N, K, idx.data_ptr(), sc.data_ptr(), None), n, K)


@pytest.mark.parametrize("K", [1, 33, 63, 64])
def test_topk_rows_every_family(pa, K):
    """poi_topk (one wavefront per row, 128 LDS slots): K = 64 on the rising staircase keeps all 128 slots in use at every compaction."""
    ctx = pa._lib.context(0)
    for N in sorted({K, 64, 65, 129, N0}):
        if N < K:
            continue
        names, S = _families(N, K)
        _assert_lists(_topk_rows(ctx, S.astype(np.float32), K), _expected(N, K), "N = %d" % N, names, np.arange(len(names)))


def _sparse_rows(N, K):
    """Rows with fewer than K selectable entries, and rows with NaN."""
    rng = np.random.default_rng(N + K)
    rows = []
    r = np.full(N, -np.inf); rows.append(r)                                               # nothing to select
    r = np.full(N, -np.inf); r[[0, N // 2, N - 1]] = [1.0, 1.0, 2.0]; rows.append(r)      # three entries (K > 3) in three ranges
    r = np.full(N, -np.inf); r[rng.choice(N, max(K - 1, 1), replace=False)] = 0.5; rows.append(r)      # K - 1 tied entries
    r = TS.mod7(N); r[::3] = np.nan; rows.append(r)                                       # NaN among ties
    r = TS.staircase_up(N); r[1::2] = np.nan; rows.append(r)
    r = np.full(N, np.nan); r[[1, N - 2]] = [-3.0, -3.0]; rows.append(r)                  # NaN everywhere else
    r = np.full(N, np.nan); rows.append(r)
    r = np.full(N, np.nan); r[::2] = -np.inf; rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize("K", [5, 32])
@pytest.mark.parametrize("N", [65, N0])
def test_short_rows_and_nan_are_never_selected(pa, N, K):
    """The contract include/poi_hip.h states for poi_topk and poi_score_topk*: an entry that is -inf or NaN is never selected; a row
    with fewer than k selectable entries ends in -1 ids and -inf scores."""
    ctx = pa._lib.context(0)
    S = _sparse_rows(N, K)
    exp = TS.expected_lists(S, K, O.topk_desc)
    assert (exp[0] == -1).any() and (exp[0][3:5] >= 0).all()
    _assert_lists(_topk_rows(ctx, S.astype(np.float32), K), exp, "poi_topk")
    if K == 32:
        _assert_lists(_topk_rows(ctx, S.astype(np.float32), 64), TS.expected_lists(S, 64, O.topk_desc), "poi_topk, k = 64")
    for n, dim in ((33, 32), (160, 32)):
        cls = np.arange(n) % S.shape[0]
        du, di = _dev(np.zeros((n, dim), np.float32)), _dev(np.ones((N, dim), np.float32))
        dp, dwd = _dev(S[cls].astype(np.float32)), _dev(np.array([1.0], np.float32))
        call = _prob_call(ctx, du, di, dwd, dp, n, N, dim, K)
        _assert_lists(_run(ctx, call, n, K), (exp[0][cls], exp[1][cls]), "poi_score_topk, n = %d" % n)
        rnd = np.stack([np.random.default_rng(u).choice(N, K, replace=False) for u in range(n)]).astype(np.int32)      # seed scores: -inf / NaN bounds
        _assert_lists(_run(ctx, call, n, K, seed=_dev(rnd)), (exp[0][cls], exp[1][cls]), "poi_score_topk seeded with random ids, n = %d" % n)


# ---- cross-contract ---------------------------------------------------------------------------------------------------------------------
def test_score_rank_of_the_topk_list_is_its_position(pa):
    """include/poi_hip.h defines poi_score_rank as "the 0-based position in an endless poi_score_topk list": on planted plateaus the
    rank of the i-th returned id must be i."""
    import torch
    ctx = pa._lib.context(0)
    n, dim, N, K = 160, 64, N0, 32
    names, full, cls, users, items, _, exp = _one_hot_problem(n, dim, N, K)
    du, di = _dev(users), _dev(items)
    call = lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
    idx, sc = _run(ctx, call, n, K, filt=False)
    _assert_lists((idx, sc), exp, "one-stage", names, cls)
    ones = torch.ones((n, 8), dtype=torch.int32, device="cuda")
    for o in range(0, K, 8):
        tgt = _dev(idx[:, o:o + 8].astype(np.int32))
        rank = torch.full((n, 8), -9, dtype=torch.int32, device="cuda")
        rsc = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.poi_score_rank(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, None, None, None, None, None, None, 0, 0.0, tgt.data_ptr(), ones.data_ptr(), 8,
                                         None, None, rank.data_ptr(), rsc.data_ptr(), None, None))
        assert np.array_equal(rank.cpu().numpy(), np.broadcast_to(np.arange(o, o + 8), (n, 8))), "ranks of list positions %d .. %d" % (o, o + 7)
        assert np.array_equal(rsc.cpu().numpy().view(np.uint32), sc[:, o:o + 8].view(np.uint32))


# ---- 16-bit item offsets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 32])
def test_item_offsets_at_the_16_bit_limit(pa, K):
    """The candidate lists hold 16-bit item offsets; splits_for caps a range at 2047 tiles = 65 504 items.  With n = 32 * 8 * num_cu users
    it asks for ONE range and the cap alone makes four: N = 4 * 2047 * 32 - 5 gives ranges of exactly 65 504 items (the last one five
    short).  Tied winners at offsets 0 and 65 503 of every range, i.e. also the first item of the next range and the last valid item.
    dim 4, one-hot over four classes: the expected lists come from the 4 x N matrix.  (Measured: docs/NOTEBOOK.md.)"""
    import torch
    ctx = pa._lib.context(0)
    R = 2047 * 32
    n, dim, N = 32 * 8 * ctx.num_cu, 4, 4 * R - 5
    j = np.arange(N)
    P = [0, R - 1, R, 2 * R - 1, 2 * R, 3 * R - 1, 3 * R, N - 1]
    S = np.tile(-8.0 - (j % 3) * 0.5, (4, 1))
    for c in range(4):
        S[c, [p + 1 for p in P[:-1]]] = 6.5                      # a second plateau right behind every winner (ties with P[7 - c])
        S[c, P] = 7.0
        S[c, P[c]] = 7.5
        S[c, P[7 - c]] = 6.5
    assert TS.is_exact(S)
    users, items, full = TS.one_hot(S, n, dim)
    eidx, esc = TS.expected_lists(full, K, O.topk_desc)
    cls = np.arange(n) % 4
    du, di = _dev(users), _dev(items)
    call = lambda idx, sc: ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, N, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = _run(ctx, call, n, K)
    print("poi_score_topk: %d users x %d items, dim 4, k = %d: %.3f s (first call: includes the context's buffer growth)" % (n, N, K, time.perf_counter() - t0))
    _assert_lists(got, (eidx[cls], esc[cls]), "four ranges of 65 504 items")
