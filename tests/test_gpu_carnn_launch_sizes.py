"""-m gpu: the CA-RNN step (poi_carnn_step, carnn.hip) against the float64 oracle at the launch sizes where its kernels change what they do.
The other CA-RNN suites stop at 59 sequences of 10 positions: no workgroup of the persistent kernels ever walks a second sequence, the scan
never gives a thread two sequences, no matrix id has more than eight 512-entry chunks, no POI row's run crosses many 64-entry windows,
no grid cap or grid-stride loop is hit.  Here, on a context of its own with the default options, every launch starts from the same
fresh-model tables (the model's own seeded init, restored from clones), in tools/bench_carnn.py's configuration - the synthetic Gowalla shape
(100 000 POIs, sequences up to 50, 80 % local transitions, launches sorted by length as bench.py sorts them) - and is held to the sparse
batch oracle (oracle/poi_oracle.py carnn_batch_step; tests/test_carnn_cpu.py ties it to carnn_step + batch_mean_update):
  * losses (assert_close), lt / wd (one row per matrix) / M to both bars of tests/gpu_util (1e-5 on the tensors, 1e-4 per row of the update);
  * the lt rows and interval matrices that changed bitwise == the ones the oracle's launch touches (a grid-stride loop that skips or
    leaves out rows shows here; a touched row whose oracle update is exactly 0 is excluded, fewer than 0.1 % of the touched rows);
  * the path, from the kernel timing regions: "carnn_outer" runs exactly when dim is 64 / 128 and n_dist + 2 <= 2048;
  * sizes, with G = num_cu * 8 (the outer-product path's grid): 1, 2, 15 | 16 (the PM-table switch: both sides must pass), 17, 1024 | 1025
    (the scan's second sequence per thread), G - 1, G, G + 1 (a workgroup's second sequence), 2 G + 3, one launch in caller order, and the
    benchmarked launch - reduced from 12 500 sequences to 3 G + 1, see below; dim 64: 1, 16, 1025, G + 1; the per-sequence kernel (dims 32
    and 256, 10 000 POIs, sequences up to 20): 1, 17, Gs + 1, 2 Gs + 3 with Gs = num_cu * wg_per_cu, and 16 num_cu + 3;
  * dim 64 with 2047 intervals (n_dist + 2 > 2048: the atomic per-sequence kernel) next to 2046 (still the outer-product path);
  * the same launch twice from identical tables: bitwise equal tables and losses (outer-product path, n = 1025 and 2 G + 3);
  * a second, different launch straight after the benchmarked one with no restore, against the oracle continued from the device's own
    tables: gradient tables, segment tables and slabs were re-zeroed at scale;
  * predict for num_cu * 4 + 5 users (more than its grid) and for every user, all-POI scores over 100 000 POIs and top-10 ranks.
The benchmarked launch: the float64 oracle takes ~14 ms per sequence on a CPU core (0.6 ms per step of rank-one updates of 128 x 128
matrices; numpy holds the interpreter lock through most of it, threads do not help), 12 500 sequences alone ~3 minutes: it is reduced to
3 G + 1, which gives the scan several sequences per thread, interval ids (not only M) more than eight chunks and every workgroup a third
and a fourth sequence - asserted from the launch's own counts (docs/NOTEBOOK.md).
G and Gs follow abi.hip with the default context options: POI_SEQ_WG_PER_CU, when set, replaces the 8 of the outer-product grid as well,
and POI_CARNN_FAST=0 (not set by any test) would take every launch off the outer-product path and fail the path assertion here.
Printed: one line per launch with its size, path and worst delta excess (<= 1 passes)."""
import math
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("lt", "wd", "M")
ALPHA, LAMBDA = 0.01, 0.001
SIZES_128 = ["1", "2", "15", "16", "17", "1024", "1025", "G-1", "G", "G+1", "2G+3", "bench"]
SIZES_64 = ["1", "16", "1025", "G+1"]
SIZES_SEQ = ["1", "17", "Gs+1", "2Gs+3", "16cu+3"]


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16), os.cpu_count() or 1))


def _wg_per_cu():
    """The per-sequence kernel's workgroups per CU as abi.hip reads them: POI_SEQ_WG_PER_CU in 1 .. 8, else 2.  The value is not observable
    through the C-ABI, so the per-sequence sizes also hold 16 num_cu + 3, which exceeds the grid at any value the library accepts."""
    try:
        v = int(os.environ.get("POI_SEQ_WG_PER_CU", ""))
    except ValueError:
        return 2
    return v if 1 <= v <= 8 else 2


def _size(label, num_cu):
    G, Gs = num_cu * (_wg_per_cu() if os.environ.get("POI_SEQ_WG_PER_CU") else 8), num_cu * _wg_per_cu()      # abi.hip poi_carnn_step
    return {"G-1": G - 1, "G": G, "G+1": G + 1, "2G+3": 2 * G + 3, "bench": 3 * G + 1, "Gs+1": Gs + 1, "2Gs+3": 2 * Gs + 3,
            "16cu+3": 16 * num_cu + 3}.get(label) or int(label)


def _flat(d):
    return {k: (np.asarray(v).reshape(np.asarray(v).shape[0], -1) if k == "wd" else np.asarray(v)) for k, v in d.items() if k in NAMES}


class Bench:
    """One OboCARNN on a context of its own with the default options; every launch starts from the same (fresh-model) tables."""

    def __init__(self, pa, ctx, model, tables, lens, n_user):
        import torch
        self.pa, self.ctx, self.m, self.tables, self.lens, self.n_user = pa, ctx, model, tables, np.asarray(lens, np.int64), n_user
        self.m.ctx = ctx
        self.init = [getattr(self.m, k).t.clone() for k in NAMES]
        self.P = self.state()
        self.dim, self.n_dist = self.P["lt"].shape[1], self.P["wd"].shape[0] - 1
        self.outer = self.dim in (64, 128) and self.n_dist + 2 <= 2048          # abi.hip poi_carnn_step: `fast`
        self.done = {}
        torch.cuda.synchronize()

    def state(self):
        P = {k: np.asarray(getattr(self.m, k).get_value(), np.float64) for k in NAMES}
        P["h0"] = np.zeros(P["lt"].shape[1])
        return P

    def users(self, n, order="sorted", seed=5):
        u = np.random.default_rng(seed).permutation(self.n_user)[:n].astype(np.int32)
        return u[np.argsort(-self.lens[u], kind="stable")] if order == "sorted" else u

    def restore(self):
        for k, t0 in zip(NAMES, self.init):
            getattr(self.m, k).t.copy_(t0)

    def launch(self, users, restore=True):
        """-> (losses, device tensors after the launch, (launches of "carnn_train", of "carnn_outer"))"""
        import torch
        if restore:
            self.restore()
        self.ctx.timing(True)
        try:
            out = np.asarray(self.m.train_batch(users))
            regions = (self.ctx.timing_get("carnn_train")[1], self.ctx.timing_get("carnn_outer")[1])
        finally:
            self.ctx.timing(False)
        torch.cuda.synchronize()
        return out, [getattr(self.m, k).t.clone() for k in NAMES], regions

    def close(self):
        self.m.ctx = self.pa._lib.context(0)
        self.ctx.close()


def _bitwise_equal(a, b):
    import torch
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


ORACLE_SECONDS = [0.0]


def _oracle(P, tables, users):
    from oracle import poi_oracle as O
    t0 = time.perf_counter()
    res = O.carnn_batch_step(P, tables, users, ALPHA, LAMBDA, threads=_threads())
    ORACLE_SECONDS[0] += time.perf_counter() - t0
    return res


def _changed_equals_touched(got, exp, old, touched, name, tag):
    """Rows that changed bitwise == rows the oracle's launch touches, but for touched rows whose oracle update is exactly zero."""
    changed = (got != old).reshape(got.shape[0], -1).any(axis=1)
    zero = touched & ~(exp != old).reshape(exp.shape[0], -1).any(axis=1)
    assert zero.sum() < 1e-3 * touched.sum(), "%s %s: %d of %d touched rows have a zero update in the oracle" % (name, tag, zero.sum(), touched.sum())
    bad = np.flatnonzero((changed != touched) & ~zero)
    assert bad.size == 0, "%s %s: %d rows changed != touched (first %s; changed but untouched %d, touched but unchanged %d)" % (
        name, tag, bad.size, bad[:8], (changed & ~touched).sum(), (touched & ~changed & ~zero).sum())


def _check(b, users, out, got, regions, P0, oracle, tag):
    """The assertions of one launch; -> worst delta excess."""
    from tests.gpu_util import assert_close, assert_step_close, delta_excess
    exp, losses, t_lt, t_wd = oracle
    assert (regions[0] > 0) and ((regions[1] > 0) == b.outer), "%s: kernel regions (train, outer) = %s, outer-product path expected: %s" % (tag, regions, b.outer)
    worst = max(delta_excess(_flat(got)[k], _flat(exp)[k], _flat(P0)[k])[0] for k in NAMES)
    print("[carnn] %-34s n %5d | dim %3d, %4d bins | path %-13s | loss error %.2e | worst delta excess %.3f" % (
        tag, len(users), b.dim, b.n_dist, "outer-product" if regions[1] else "per-sequence", np.abs(out - losses).max() / max(np.abs(losses).max(), 1e-30), worst), flush=True)
    assert_close(out, losses, "losses " + tag)
    assert_step_close(_flat(got), _flat(exp), _flat(P0), NAMES, tag)
    _changed_equals_touched(got["lt"], exp["lt"], P0["lt"], t_lt, "lt", tag)
    _changed_equals_touched(got["wd"], exp["wd"], P0["wd"], t_wd, "wd", tag)
    return worst


def _run(b, n, order="sorted", tag="", keep=False):
    """One launch of n sequences from the fresh tables against the oracle (one per size: a repeated size is the same launch)."""
    key = (n, order)
    if key in b.done:
        return b.done[key]
    users = b.users(n, order)
    out, tabs, regions = b.launch(users)
    got = b.state()
    if (n, "oracle") in b.done:           # the same users in another order: the batch rule is a mean per row, the order only permutes the losses
        users0, oracle = b.done[(n, "oracle")]
        pos = {int(u): i for i, u in enumerate(users0)}
        oracle = (oracle[0], oracle[1][[pos[int(u)] for u in users]]) + oracle[2:]
    else:
        oracle = _oracle(b.P, b.tables, users)
        if keep:
            b.done[(n, "oracle")] = (users, oracle)
    _check(b, users, out, got, regions, b.P, oracle, "%s %s" % (tag, order))
    b.done[key] = (users, out, tabs, regions)
    return b.done[key]


# ---- the Gowalla shape: dims 128 and 64 on the outer-product path ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


@pytest.fixture(scope="module")
def gowalla(pa):
    """(dataset, CSR tables, num_cu): tools/bench_carnn.py's shape with bench.py's 80 % local transitions, as many users as the largest
    launch needs."""
    from poi_amd import data as pdata
    ctx = pa._lib.Context(0)
    num_cu = ctx.num_cu
    ctx.close()
    n_item, _, max_len, _ = pdata.SHAPES["gowalla"]
    n_user = max(_size(l, num_cu) for l in SIZES_128)
    ds = pdata.make_synthetic(n_user, n_item, max_len, seed=20260930, local=0.8)
    assert ds.dist_num == 200 and ds.len_max == 50
    return ds, ds.shard(0, n_user), num_cu


def _carnn_bench(pa, ds, tab, D, seed):
    m = pa.models.OboCARNN(train=tab, test=None, dist=None, alpha_lambda=[ALPHA, LAMBDA], n_user=ds.n_user, n_item=ds.n_item,
                           n_dists=[ds.dist_num, ds.dd / 1000.0], n_in=D, n_hidden=D, seed=seed, coords=ds.coords)
    return Bench(pa, pa._lib.Context(0), m, tab, np.diff(tab.off.astype(np.int64)), ds.n_user)


@pytest.fixture(scope="module")
def g128(pa, gowalla):
    ds, tab, _ = gowalla
    b = _carnn_bench(pa, ds, tab, 128, 7)
    yield b
    print("[carnn] float64 oracle so far: %.0f s on %d threads" % (ORACLE_SECONDS[0], _threads()))
    b.close()


@pytest.fixture(scope="module")
def g64(pa, gowalla):
    ds, tab, _ = gowalla
    b = _carnn_bench(pa, ds, tab, 64, 8)
    yield b
    b.close()


@pytest.mark.parametrize("label", SIZES_128)
def test_dim128_launch_matches_the_oracle(g128, gowalla, label):
    n = _size(label, gowalla[2])
    _run(g128, n, "sorted", "gowalla d128 %s" % label, keep=(label == "2G+3"))
    assert g128.outer


def test_dim128_benchmarked_launch_reaches_what_it_was_reduced_for(g128, gowalla):
    """The reduced benchmark launch (module docstring), from the oracle's own counts: two sequences per scan thread, a matrix id with more
    than eight 512-entry chunks, more than two sequences per workgroup; and POI rows whose runs cross many 64-entry windows."""
    ds, tab, num_cu = gowalla
    n = _size("bench", num_cu)
    users = g128.users(n)
    off = tab.off.astype(np.int64)
    steps = np.maximum(g128.lens[users] - 1, 0)
    per = (n + 1023) // 1024
    assert per >= 2 and n > 2 * _size("G", num_cu)
    # entries per matrix id (carnn_train2_kernel): dp[t + 1], dq[t + 1], dp[t] for every step, and three for M
    ent = np.zeros(ds.dist_num + 2, np.int64)
    rows = np.zeros(ds.n_item + 1, np.int64)
    for u in users:
        a, e = off[u], off[u + 1]
        if e - a < 2:
            continue
        np.add.at(ent, tab.dp[a + 1:e], 1); np.add.at(ent, tab.dq[a + 1:e], 1); np.add.at(ent, tab.dp[a:e - 1], 1)
        np.add.at(rows, tab.p[a + 1:e], 1); np.add.at(rows, tab.q[a + 1:e], 1); np.add.at(rows, tab.p[a:e - 1], 1)
    ent[-1] = 3 * steps.sum()
    chunks = (ent + 511) // 512
    print("[carnn] benchmarked launch n %d: %d steps, scan %d per thread, chunks per id max %d (M) / %d (largest interval id), interval ids over 8 chunks: %d, "
          "longest POI-row run %d entries" % (n, steps.sum(), per, chunks[-1], chunks[:-1].max(), (chunks[:-1] > 8).sum(), rows.max()))
    assert chunks[-1] > 8 and (chunks[:-1] > 8).sum() >= 1      # M and at least one interval id: the owner search of ca_outer_kernel crosses multi-chunk ids
    assert rows.max() > 4 * 64


def test_dim128_launch_in_caller_order(g128, gowalla):
    n = _size("2G+3", gowalla[2])
    _run(g128, n, "sorted", "gowalla d128 2G+3", keep=True)
    _run(g128, n, "caller", "gowalla d128 2G+3")


@pytest.mark.parametrize("label", ["1025", "2G+3"])
def test_dim128_identical_launches_are_bitwise_equal(g128, gowalla, label):
    n = _size(label, gowalla[2])
    users, out, tabs, regions = _run(g128, n, "sorted", "gowalla d128 %s" % label, keep=(label == "2G+3"))
    out2, tabs2, regions2 = g128.launch(users)
    assert regions2 == regions
    assert _bitwise_equal(tabs, tabs2), "n = %d: tables differ between identical launches" % n
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "n = %d: losses differ between identical launches" % n


def test_dim128_second_launch_without_restore(g128, gowalla):
    """The benchmarked launch, then - tables as it left them - a different launch of G + 1 sequences against the oracle continued from the
    device's own (float32) tables."""
    from tests.gpu_util import round_f32
    b, num_cu = g128, gowalla[2]
    n = _size("bench", num_cu)
    out, tabs, regions = b.launch(b.users(n))
    P1 = round_f32(b.state())
    users2 = b.users(_size("G+1", num_cu), seed=11)
    out2, tabs2, regions2 = b.launch(users2, restore=False)
    _check(b, users2, out2, b.state(), regions2, P1, _oracle(P1, b.tables, users2), "gowalla d128 G+1 after bench")


@pytest.mark.parametrize("label", SIZES_64)
def test_dim64_launch_matches_the_oracle(g64, gowalla, label):
    _run(g64, _size(label, gowalla[2]), "sorted", "gowalla d64 %s" % label)
    assert g64.outer


# ---- the per-sequence kernel: dim 32, and dim 256 (accepted by poi_carnn_step, run by no other test) ---------------------------------------------
@pytest.fixture(scope="module")
def small(pa, gowalla):
    from poi_amd import data as pdata
    n_user = 16 * gowalla[2] + 3
    ds = pdata.make_synthetic(n_user, 10_000, 20, seed=20260931, local=0.8)
    return ds, ds.shard(0, n_user)


@pytest.fixture(scope="module")
def s32(pa, small):
    b = _carnn_bench(pa, small[0], small[1], 32, 9)
    yield b
    b.close()


@pytest.fixture(scope="module")
def s256(pa, small):
    b = _carnn_bench(pa, small[0], small[1], 256, 10)
    yield b
    b.close()


@pytest.mark.parametrize("label", SIZES_SEQ)
def test_dim32_per_sequence_launch_matches_the_oracle(s32, gowalla, label):
    _run(s32, _size(label, gowalla[2]), "sorted", "10k d32 %s" % label)
    assert not s32.outer


@pytest.mark.parametrize("label", SIZES_SEQ)
def test_dim256_per_sequence_launch_matches_the_oracle(s256, gowalla, label):
    _run(s256, _size(label, gowalla[2]), "sorted", "10k d256 %s" % label)
    assert not s256.outer


# ---- dim 64 beyond the id table of the outer-product path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dist,outer", [(2046, True), (2047, False)])
def test_dim64_falls_back_to_the_per_sequence_kernel_above_2048_ids(pa, n_dist, outer):
    """n_dist + 2 <= 2048 is the outer-product path's limit (ca_chunks_kernel's id table): 2046 intervals stay on it, 2047 take the
    per-sequence kernel with float atomics.  64 sequences on a toy table (wd is 2048 x 64 x 64 floats)."""
    from oracle import poi_oracle as O
    from tests.gpu_util import round_f32, toy_problem
    T = toy_problem(560, n_user=70, n_item=300, n_dist=n_dist, dim=64, len_max=12, hot=60, min_len=1)
    P = round_f32(O.init_carnn_params(np.random.default_rng(560 + n_dist), T["n_item"], n_dist, 64))
    m = pa.models.OboCARNN(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[ALPHA, LAMBDA], n_user=70, n_item=300,
                           n_dists=[n_dist, 0.2], n_in=64, n_hidden=64, init=P)
    b = Bench(pa, pa._lib.Context(0), m, (T["train"][0], T["train"][2], T["dist"][0], T["dist"][2], T["train"][1]), T["lens"], 70)
    try:
        assert b.outer == outer
        _run(b, 64, "caller", "toy d64")
    finally:
        b.close()


# ---- predict and scoring at scale -----------------------------------------------------------------------------------------------------------------
def _bins_vectorised(last, coords, dd, dist_num):
    """oracle.poi_oracle.compute_distance / cal_dis for the rows `last` (each user's last train POI) against every POI, whole arrays at a
    time: the same float64 expression in the same order, cos / asin / sqrt through the scalar libm routines cal_dis calls."""
    f = lambda fn, x: np.frompyfunc(fn, 1, 1)(x).astype(np.float64)
    d, p = 12742, 0.017453292519943295
    lat1, lon1 = coords[last, 0][:, None], coords[last, 1][:, None]
    lat2, lon2 = coords[:, 0][None, :], coords[:, 1][None, :]
    a = (lat1 - lat2) * p
    b = (lon1 - lon2) * p
    c = (1.0 - f(math.cos, a)) / 2 + f(math.cos, lat1 * p) * f(math.cos, lat2 * p) * (1.0 - f(math.cos, b)) / 2
    dist = d * f(math.asin, f(math.sqrt, c))
    return np.minimum((dist * 1000 / dd).astype(np.int64), dist_num)


SCORE_USERS_SEED = 4           # (checked with the oracle alone, 256 CUs: all 8 rows keep top-11 gaps above 1e-5 max|score|, the smallest 5x over)


def test_predict_scores_and_topk_at_scale(g128, gowalla):
    """seq_predict for more users than carnn_predict_kernel's grid (num_cu * 4), all-POI scores over 100 000 POIs with the dataset's 200
    intervals (many blocks and trips of carnn_score_kernel) for 8 users, top-10 ranks on gap-checked rows.  The predicted states
    saturate at this shape (sum(h) enters every unit, public/CA_RNN.py:191): every user's sum is the same 128, so the scores and ranks are
    checked on the model's own seeded user rows (uniform, distinct sums) as well as on the predicted ones."""
    from oracle import poi_oracle as O
    from tests.gpu_util import assert_close
    ds, tab, num_cu = gowalla
    b, m, P = g128, g128.m, g128.P
    b.restore()
    m.update_trained_items(); m.update_trained_dists()
    pad = ds.to_padded()
    Pm, Mm, DPm = pad["train"][0], pad["train"][1], pad["dist"][0]
    ids = np.random.default_rng(21).permutation(ds.n_user)[:num_cu * 4 + 5].astype(np.int32)
    hts = m.predict(ids)
    assert_close(hts, O.carnn_predict(P, P["lt"], P["wd"], Pm[ids], DPm[ids], Mm[ids]), "hts of %d users" % len(ids))
    every = np.arange(ds.n_user, dtype=np.int32)
    hts_all = m.predict(every)
    assert_close(hts_all, O.carnn_predict(P, P["lt"], P["wd"], Pm, DPm, Mm), "hts of every user")
    # the same two calls on a snapshot that does not saturate: interval matrices scaled to 0.1 wd - 7 / D, whose row sums (about -7) keep
    # every unit near exp(-7 +- 1) and sum(h) below 1 - each user's state then depends on its own POIs and bins, a grid-stride loop that
    # read another user's sequence would show
    D = P["lt"].shape[1]
    m.trained_dists.set_value(0.1 * P["wd"] - 7.0 / D)
    try:
        W = np.asarray(m.trained_dists.get_value(), np.float64)
        exp_ids, exp_all = O.carnn_predict(P, P["lt"], W, Pm[ids], DPm[ids], Mm[ids]), O.carnn_predict(P, P["lt"], W, Pm, DPm, Mm)
        assert ((exp_all > 1e-5) & (exp_all < 0.5)).mean() > 0.99, "the scaled snapshot saturates"
        top = exp_all.max(axis=1)
        assert top.std() > 0.1 * top.mean(), "the users' states do not differ"
        assert_close(m.predict(ids), exp_ids, "unsaturated hts of %d users" % len(ids))
        assert_close(m.predict(every), exp_all, "unsaturated hts of every user")
    finally:
        m.update_trained_dists()
    # the bins of (last train POI, POI): the vectorised restatement is the oracle's, bit for bit
    cor = [tuple(c) for c in ds.coords[:500]]
    sub3 = np.array([0, 1, 2])
    small_p = np.minimum(Pm[sub3], 499)
    last3 = small_p[np.arange(3), Mm[sub3].sum(axis=1) - 1]
    assert np.array_equal(_bins_vectorised(last3, ds.coords[:500], ds.dd, ds.dist_num), O.compute_distance(small_p, Mm[sub3], cor, ds.dd, ds.dist_num))
    sub = np.sort(np.random.default_rng(SCORE_USERS_SEED).permutation(ds.n_user)[:8]).astype(np.int32)
    bins = _bins_vectorised(ds.last_pois()[sub], ds.coords, ds.dd, ds.dist_num)
    assert bins.shape == (8, 100_000) and len(np.unique(bins)) > 100
    for what, rows in (("seeded user rows", np.asarray(m.trained_users.get_value(), np.float64)), ("predicted user rows", np.asarray(hts_all, np.float64))):
        m.update_trained_users(rows)
        sc = m.compute_sub_all_scores(sub)
        full = O.carnn_score_all(np.asarray(m.trained_users.get_value(), np.float64)[sub], P["lt"], P["M"], P["wd"], bins)
        assert sc.shape == (8, 100_000)
        assert_close(sc, full, "scores, " + what)
        if what == "seeded user rows":
            idx = m.compute_sub_topk(sub, 10).cpu().numpy()
            top = O.topk_desc(full, 11)
            tv = np.take_along_axis(full, top, axis=1)
            ok = (tv[:, :-1] - tv[:, 1:]).min(axis=1) > 1e-5 * np.abs(tv).max()
            assert ok.mean() >= 0.9, ok
            assert np.array_equal(idx[ok], top[ok][:, :10])
