"""-m gpu tests of the label recommendation (poi_score_labels, poi_score_topk_labels, poi_labels_scores ->
models.recommend_labels / label_distribution, Session.recommend_labels, evaluate.label_hit_rate).  The accumulators are held TIGHTLY to
the numpy oracle of tests/labels_oracle.py run on the device's own float32 rows (poi_score_rows): best POI and count exactly, the
integer mass to one rounding unit per term; the log-probabilities and the label lists to the float64 oracle, independently of the
project's own score rows, on the rows that oracle leaves clear; every grid, regime, accumulator home, chunking and call size gives the
same bits; and the edges - unlabelled POIs, empty labels, emptied rows, planted ties, NaN and -inf columns, a half table, bad rows."""
import ctypes

import numpy as np
import pytest

from tests import filter_oracle as FO
from tests import labels_cases as LC
from tests import labels_oracle as LO
from tests.gpu_util import RTOL
from tests.test_gpu_filter import dev, dev_ex, p, same_bits

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -1, -4
BY = {"mass": 0, "max": 1}
LOG_ATOL = 2e-14      # two float64 logs near 36 log 2 = 25 (half an ulp of 3.6e-15 each, twice: two libraries) and their difference
DENSE = ("mass", "best_id", "best_score", "count", "M", "lognorm")
TOPK = ("label", "logp", "best_id", "best_score", "n_listed", "rest_logp", "M", "lognorm")


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def reset(c):
    c.set_option("labels_split_max", 256); c.set_option("labels_grid", 0); c.set_option("labels_lds_kb", 40); c.set_option("labels_ws_kb", 256 << 10)


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa._lib.context(0)
    yield c
    reset(c)


class Dev:
    """A case of tests/labels_cases.py on the device, with everything a raw call needs."""

    def __init__(self, C, items=None):
        self.C, self.N, self.L, self.dim, self.n = C, C["n_item"], C["n_label"], C["dim"], LC.N_ROWS
        self.users, self.items, self.labels = dev(C["users"]), dev(C["items"]) if items is None else items, dev(C["labels"])
        g = C["geo"]
        self.geo = None if g is None else dict(wd=dev(np.array([g["wd"]], np.float32)), sts=dev(g["sts"]), coords=dev(g["coords"]), cphi=dev(g["cphi"]),
                                               thr=dev(g["thr"]), anchor=dev(g["anchor"].astype(np.int32)), n_dist=g["n_dist"], dd_m=g["dd_m"])

    def operands(self, rows, anchor=None):
        """The 13 arguments users .. dd of a fused entry for the rows `rows` (+ the tensors, kept alive by the caller)."""
        sel = dev(np.asarray(rows, np.int64))
        users = self.users.index_select(0, sel).contiguous()
        g = self.geo
        if g is None:
            anc = None if anchor is None else dev(np.asarray(anchor, np.int32))
            return [p(users), p(self.items), len(rows), self.N, self.dim, None, None, None, None, None, p(anc), 0, 0.0], (users, sel, anc)
        sts = g["sts"].index_select(0, sel).contiguous()
        anc = g["anchor"].index_select(0, sel).contiguous() if anchor is None else dev(np.asarray(anchor, np.int32))
        return [p(users), p(self.items), len(rows), self.N, self.dim, p(g["wd"]), p(sts), p(g["coords"]), p(g["cphi"]), p(g["thr"]), p(anc), g["n_dist"],
                g["dd_m"]], (users, sel, sts, anc)

    def ex_of(self, rows, ex):
        return LC.sub_lists(self.C["ex"], rows) if isinstance(ex, str) else ex


def dense_buffers(n, L1):
    import torch
    return dict(mass=torch.full((n, L1), -7, dtype=torch.int64, device="cuda"), best_id=torch.full((n, L1), -7, dtype=torch.int32, device="cuda"),
                best_score=torch.full((n, L1), 7.0, dtype=torch.float32, device="cuda"), count=torch.full((n, L1), -7, dtype=torch.int32, device="cuda"),
                M=torch.full((n,), 7.0, dtype=torch.float32, device="cuda"), lognorm=torch.full((n,), 7.0, dtype=torch.float64, device="cuda"))


def topk_buffers(n, k):
    import torch
    k = max(k, 1)
    return dict(label=torch.full((n, k), -7, dtype=torch.int32, device="cuda"), logp=torch.full((n, k), 7.0, dtype=torch.float64, device="cuda"),
                best_id=torch.full((n, k), -7, dtype=torch.int32, device="cuda"), best_score=torch.full((n, k), 7.0, dtype=torch.float32, device="cuda"),
                n_listed=torch.full((n,), -7, dtype=torch.int32, device="cuda"), rest_logp=torch.full((n,), 7.0, dtype=torch.float64, device="cuda"),
                M=torch.full((n,), 7.0, dtype=torch.float32, device="cuda"), lognorm=torch.full((n,), 7.0, dtype=torch.float64, device="cuda"))


def host(bufs):
    out = {k: t.cpu().numpy() for k, t in bufs.items()}
    if "mass" in out:
        out["mass"] = out["mass"].view(np.uint64)
    return out


def dense_call(ctx, V, rows=None, ex="own", labels=None, n_label=None, anchor=None, expect=0):
    """poi_score_labels on the rows `rows` of a Dev (default: all) -> dict of numpy arrays, or the error code."""
    rows = np.arange(V.n) if rows is None else np.asarray(rows)
    ops, keep = V.operands(rows, anchor)
    exd = dev_ex(V.ex_of(rows, ex))
    L = V.L if n_label is None else n_label
    B = dense_buffers(len(rows), L + 1)
    rc = ctx.lib.poi_score_labels(ctx.handle, *ops, p(V.labels if labels is None else labels), L, p(exd[0]), p(exd[1]), p(B["mass"]), p(B["best_id"]),
                                  p(B["best_score"]), p(B["count"]), p(B["M"]), p(B["lognorm"]), None)
    if expect:
        assert rc == expect, (rc, expect)
        return rc
    ctx.check(rc)
    return host(B)


def topk_call(ctx, V, by, k, rows=None, ex="own", labels=None, n_label=None, anchor=None, expect=0):
    rows = np.arange(V.n) if rows is None else np.asarray(rows)
    ops, keep = V.operands(rows, anchor)
    exd = dev_ex(V.ex_of(rows, ex))
    B = topk_buffers(len(rows), k)
    rc = ctx.lib.poi_score_topk_labels(ctx.handle, *ops, p(V.labels if labels is None else labels), V.L if n_label is None else n_label, p(exd[0]),
                                       p(exd[1]), BY.get(by, by), k, p(B["label"]), p(B["logp"]), p(B["best_id"]), p(B["best_score"]), p(B["n_listed"]),
                                       p(B["rest_logp"]), p(B["M"]), p(B["lognorm"]), None)
    if expect:
        assert rc == expect, (rc, expect)
        return rc
    ctx.check(rc)
    return host(B)


def scores_call(ctx, sc, N, labels, n_label, ex=(None, None), by="mass", k=0, expect=0):
    """poi_labels_scores on device score rows sc (n, ld) -> (dense dict, top-K dict or None), or the error code."""
    n = sc.shape[0]
    exd = dev_ex(ex)
    B, T = dense_buffers(n, n_label + 1), topk_buffers(n, k)
    rc = ctx.lib.poi_labels_scores(ctx.handle, p(sc), n, N, sc.shape[1], p(labels), n_label, p(exd[0]), p(exd[1]), BY.get(by, by), k, p(B["mass"]),
                                   p(B["best_id"]), p(B["best_score"]), p(B["count"]), p(T["label"]), p(T["logp"]), p(T["best_id"]), p(T["best_score"]),
                                   p(T["n_listed"]), p(T["rest_logp"]), p(B["M"]), p(B["lognorm"]), None)
    if expect:
        assert rc == expect, (rc, expect)
        return rc
    ctx.check(rc)
    T.pop("M"); T.pop("lognorm")
    return host(B), (host(T) if k else None)


def score_rows(ctx, V, rows=None):
    """The device's own float32 score rows (poi_score_rows) -> (device tensor (n, n_item), numpy)."""
    import torch
    rows = np.arange(V.n) if rows is None else np.asarray(rows)
    ops, keep = V.operands(rows)
    out = torch.empty((len(rows), V.N), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.poi_score_rows(ctx.handle, *ops, p(out), V.N, None))
    return out, out.cpu().numpy()


def bits_equal(a, b, what, keys=None):
    for key in (keys or a.keys()):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs" % (what, key)


def assert_tight(got, want, what):
    """Device accumulators against the oracle on the same float32 rows: best and count exactly, |mass difference| <= count."""
    assert np.array_equal(got["count"], want["count"]), "%s: counts" % what
    assert np.array_equal(got["best_id"], want["best_id"]), "%s: best ids" % what
    assert same_bits(got["best_score"], want["best_score"].astype(np.float32)), "%s: best scores" % what
    assert same_bits(got["M"], want["M"].astype(np.float32)), "%s: M" % what
    d = np.abs(got["mass"].astype(np.int64) - want["mass"].astype(np.int64))
    print("%s: max |mass_q difference| %d units (max count %d)" % (what, d.max(initial=0), want["count"].max(initial=0)))
    assert (d <= want["count"]).all(), "%s: mass off by more than one unit per term" % what


def assert_topk_of_dense(T, D, by, k, what):
    """A top-K result against the dense result of the same call: the list is the oracle's order of the DEVICE's masses / bests, the
    bests bit for bit, log p within two float64 log roundings."""
    Dd = dict(D, total=D["mass"].sum(axis=1, dtype=np.uint64))
    W = LO.topk(Dd, by, k)
    assert np.array_equal(T["label"], W["label"]) and np.array_equal(T["n_listed"], W["n_listed"]), "%s: labels" % what
    assert np.array_equal(T["best_id"], W["best_id"]) and same_bits(T["best_score"], W["best_score"]), "%s: bests" % what
    for key in ("logp", "rest_logp"):
        fin = np.isfinite(W[key])
        assert np.array_equal(np.isneginf(T[key]), ~fin) and np.abs(T[key][fin] - W[key][fin]).max(initial=0) <= LOG_ATOL, "%s: %s" % (what, key)
    assert same_bits(T["M"], D["M"]) and np.array_equal(T["lognorm"].view(np.uint64), D["lognorm"].view(np.uint64)), "%s: M / lognorm" % what
    ln = LO.lognorm(dict(Dd, M=D["M"]))
    fin = np.isfinite(ln)
    assert np.array_equal(np.isneginf(D["lognorm"]), ~fin) and np.abs(D["lognorm"][fin] - ln[fin]).max(initial=0) <= 4 * LOG_ATOL, "%s: lognorm" % what


@pytest.fixture(scope="module")
def devs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Dev(LC.case(name))
        return cache[name]
    return get


# ---- 1: the tight check on the device's own rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.CASES))
def test_accumulators_are_the_oracle_on_the_devices_own_rows(ctx, devs, name):
    reset(ctx)
    V = devs(name)
    C = V.C
    _, rows32 = score_rows(ctx, V)
    for ex, mask in (("own", LC.ex_mask(C)), ((None, None), None)):
        want = LO.dense(rows32, mask, C["labels"], V.L)
        got = dense_call(ctx, V, ex=ex)
        assert_tight(got, want, "%s lists %s" % (name, ex == "own"))
        for by in ("mass", "max"):
            for k in sorted({1, C["k"], 32}):
                assert_topk_of_dense(topk_call(ctx, V, by, k, ex=ex), got, by, k, "%s by %s k %d" % (name, by, k))
    assert ctx.take_bad_ids() == 0
    assert ctx.last_plan("labels_home") == (1 if 32 * (V.L + 1) * 20 <= 40 << 10 else 2) and ctx.last_plan("labels_splits") > 0


# ---- 2: the float64 model oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.CASES))
def test_log_probabilities_and_lists_against_the_float64_oracle(ctx, devs, name):
    reset(ctx)
    V = devs(name)
    C = V.C
    osc = LC.oracle_scores(name)
    tol = RTOL * max(1.0, float(np.abs(osc).max()))
    D64 = LO.dense(osc, LC.ex_mask(C), C["labels"], V.L)
    got = dense_call(ctx, V)
    # every label's log-probability, from the device's dense masses, and the normaliser
    lp64 = LO.log_share(D64["mass"], D64["total"][:, None])
    lp = LO.log_share(got["mass"], got["mass"].sum(axis=1, dtype=np.uint64)[:, None])
    live = np.isfinite(lp64)
    assert np.array_equal(np.isfinite(lp), live) and np.array_equal(got["count"], D64["count"])
    print("%s: max |log p - oracle| %.3g, max |lognorm - oracle| %.3g (bound %.3g)" % (name, np.abs(lp[live] - lp64[live]).max(),
                                                                                 np.abs(got["lognorm"] - LO.lognorm(D64)).max(), tol))
    assert np.abs(lp[live] - lp64[live]).max() <= tol
    assert np.abs(got["lognorm"] - LO.lognorm(D64)).max() <= tol and np.abs(got["M"] - D64["M"]).max() <= tol
    for by in ("mass", "max"):
        k = C["k"]
        W = LO.topk(D64, by, k)
        T = topk_call(ctx, V, by, k)
        clear = LO.clear_rows(D64, osc, by, k)
        print("%s by %s: %.1f %% of %d rows clear" % (name, by, 100 * clear.mean(), len(clear)))
        assert clear.mean() >= 0.9
        assert np.array_equal(T["label"][clear], W["label"][clear]) and np.array_equal(T["best_id"][clear], W["best_id"][clear]), (name, by)
        assert np.array_equal(T["n_listed"], W["n_listed"])
        fin = clear[:, None] & np.isfinite(W["logp"])
        assert np.abs(T["logp"][fin] - W["logp"][fin]).max(initial=0) <= tol and np.abs(T["best_score"][fin] - W["best_score"][fin]).max(initial=0) <= tol
        rest = np.isfinite(W["rest_logp"])
        assert np.array_equal(np.isfinite(T["rest_logp"]), rest) and np.abs(T["rest_logp"][rest] - W["rest_logp"][rest]).max(initial=0) <= tol


# ---- 3: bit identities --------------------------------------------------------------------------------------------------------------------
def all_outputs(ctx, V, rows=None, k=None, ex="own"):
    k = V.C["k"] if k is None else k
    return dense_call(ctx, V, rows, ex), topk_call(ctx, V, "mass", k, rows, ex), topk_call(ctx, V, "max", k, rows, ex)


def assert_same_outputs(a, b, what, rows=None):
    for x, y, keys in zip(a, b, (DENSE, TOPK, TOPK)):
        bits_equal(x if rows is None else {key: x[key][rows] for key in keys}, y, what, keys)


@pytest.mark.parametrize("name", ["cat37", "grid1681", "geo11", "tiny27"])
def test_every_grid_regime_home_chunking_and_call_size_gives_the_same_bits(ctx, devs, name):
    reset(ctx)
    V = devs(name)
    ref = all_outputs(ctx, V)
    homes = set()
    try:
        for split_max, grid in ((0, 0), (256, 1), (256, 3), (256, 64)):              # the tile regime, then 1 / 3 / 64 slices
            for lds_kb in (0, 120):                                                  # both homes where the labels fit LDS at all
                ctx.set_option("labels_split_max", split_max); ctx.set_option("labels_grid", grid); ctx.set_option("labels_lds_kb", lds_kb)
                assert_same_outputs(all_outputs(ctx, V), ref, "%s split_max %d grid %d lds %d" % (name, split_max, grid, lds_kb))
                assert ctx.last_plan("labels_splits") == (grid if split_max else 0)
                homes.add(ctx.last_plan("labels_home"))
        assert homes == ({1, 2} if 32 * (V.L + 1) * 20 <= 120 << 10 else {2})
        reset(ctx)
        ctx.set_option("labels_ws_kb", 1)                                            # one 32-row tile at a time: five chunks
        assert_same_outputs(all_outputs(ctx, V), ref, "%s chunked" % name)
        assert ctx.last_plan("labels_chunks") == 5 and ctx.last_plan("labels_rows_per_chunk") == 32
        reset(ctx)
        assert_same_outputs(all_outputs(ctx, V), ref, "%s again" % name)
        for rows in ([5], [143], np.arange(20, 53)):                                 # a row alone; 33 rows
            assert_same_outputs(ref, all_outputs(ctx, V, rows), "%s rows %s" % (name, rows[:2]), rows=np.asarray(rows))
    finally:
        reset(ctx)
    assert ctx.take_bad_ids() == 0


@pytest.mark.parametrize("name", ["zipf37", "geo200"])
def test_integer_identities_of_the_mass(ctx, devs, name):
    """The buckets sum to the one-label total; the mass under an exclusion list is the mass without it minus the listed POIs' own
    terms - exact integers, the terms read off a call in which every POI is a label of its own."""
    reset(ctx)
    V = devs(name)
    C = V.C
    full, cut = dense_call(ctx, V, ex=(None, None)), dense_call(ctx, V)
    one = dense_call(ctx, V, ex=(None, None), labels=dev(np.zeros(V.N, np.int32)), n_label=1)
    assert np.array_equal(full["mass"].sum(axis=1, dtype=np.uint64), one["mass"][:, 0]) and not one["mass"][:, 1].any()
    assert np.array_equal(full["count"].sum(axis=1), one["count"][:, 0]) and (one["count"][:, 0] == V.N).all()
    assert same_bits(one["M"], full["M"]) and same_bits(cut["M"], full["M"])          # M does not depend on the lists
    own = dense_call(ctx, V, ex=(None, None), labels=dev(np.arange(V.N, dtype=np.int32)), n_label=V.N)
    q = own["mass"][:, :V.N]                                                          # q(r, j) as the device computes it
    assert (own["count"][:, :V.N] == 1).all() and np.array_equal(own["best_id"][:, :V.N], np.tile(np.arange(V.N), (V.n, 1)))
    b = LO.buckets(C["labels"], V.L)
    off, ids = C["ex"]
    want = full["mass"].copy()
    for r in range(V.n):
        j = ids[off[r]:off[r + 1]]
        np.subtract.at(want[r], b[j], q[r, j])
    assert np.array_equal(cut["mass"], want)


@pytest.mark.parametrize("name", ["cat37", "geo11", "many700"])
def test_by_max_is_the_capped_entry_at_per_one(ctx, devs, name):
    """Labels, ids and scores of poi_score_topk_capped(per = 1), bit for bit (labellings without unlabelled POIs)."""
    import torch
    reset(ctx)
    V = devs(name)
    assert (V.C["labels"] >= 0).all()
    for rows in (np.arange(V.n), np.arange(33)):
        for k in (1, V.C["k"], 32):
            T = topk_call(ctx, V, "max", k, rows)
            ops, keep = V.operands(rows)
            exd = dev_ex(V.ex_of(rows, "own"))
            idx = torch.full((len(rows), k), -7, dtype=torch.int32, device="cuda")
            val = torch.full((len(rows), k), 7.0, dtype=torch.float32, device="cuda")
            lab = torch.full((len(rows), k), -7, dtype=torch.int32, device="cuda")
            ctx.check(ctx.lib.poi_score_topk_capped(ctx.handle, *ops, p(V.labels), 1, None, None, 0, 0, None, p(exd[0]), p(exd[1]), k, p(idx), p(val), p(lab),
                                                    None, None))
            assert np.array_equal(T["label"], lab.cpu().numpy()) and np.array_equal(T["best_id"], idx.cpu().numpy()), (name, k)
            assert same_bits(T["best_score"], val.cpu().numpy()), (name, k)


@pytest.mark.parametrize("name", ["zipf37", "grid1681", "geo200"])
def test_the_fused_entries_are_the_explicit_rows_entry_on_their_own_rows(ctx, devs, name):
    import torch
    reset(ctx)
    V = devs(name)
    sc, _ = score_rows(ctx, V)
    padded = torch.cat([sc, torch.full((V.n, 3), 1e30, device="cuda")], 1).contiguous()      # ld > n_item: three columns never read
    try:
        for lds_kb in (40, 0):
            ctx.set_option("labels_lds_kb", lds_kb)
            for by in ("mass", "max"):
                D, T = scores_call(ctx, padded, V.N, V.labels, V.L, V.C["ex"], by, V.C["k"])
                assert ctx.last_plan("labels_home") == (1 if lds_kb else 2)          # (one row per workgroup: 1682 buckets fit 40 KiB)
                bits_equal(D, dense_call(ctx, V), "%s dense (lds %d)" % (name, lds_kb), DENSE)
                bits_equal(T, topk_call(ctx, V, by, V.C["k"]), "%s by %s (lds %d)" % (name, by, lds_kb), TOPK[:6])
    finally:
        reset(ctx)
    assert ctx.take_bad_ids() == 0


# ---- 4: edges -----------------------------------------------------------------------------------------------------------------------------
def test_planted_ties_nan_and_inf_columns(ctx):
    """Exact integer products: ties in the best score across labels (the lower id wins) and in the mass (equal score multisets: the
    lower label first), a NaN column and a -inf entry that are no candidates, zeros of both signs."""
    reset(ctx)
    users, items, sc, lab = LC.tie_tables()
    V = Dev(dict(users=np.tile(users, (5, 1))[:LC.N_ROWS], items=items, labels=lab, n_label=7, n_item=1003, dim=32, geo=None, ex=FO.csr([[]] * LC.N_ROWS), k=7))
    want = LO.dense(np.tile(sc, (5, 1))[:LC.N_ROWS], None, lab, 7)
    got = dense_call(ctx, V, ex=(None, None))
    assert_tight(got, want, "tie tables")
    assert (got["count"].sum(axis=1) == 1003 - 2).all()
    assert got["mass"][0, 0] == got["mass"][0, 1] > 0
    for by in ("mass", "max"):
        T = topk_call(ctx, V, by, 7, ex=(None, None))
        assert_topk_of_dense(T, got, by, 7, "tie tables by %s" % by)
        assert (T["n_listed"] == 7).all()
    at = topk_call(ctx, V, "mass", 7, ex=(None, None))["label"][0].tolist()
    assert at.index(0) + 1 == at.index(1)
    # explicit rows with a +inf score, an all-NaN row and a row of -inf: non-finite M - fill
    rows = np.tile(sc[:4], (1, 1)).copy()
    rows[0, 17] = np.inf; rows[1] = np.nan; rows[2] = -np.inf
    D, T = scores_call(ctx, dev(rows), 1003, dev(lab), 7, by="mass", k=7)
    assert np.isposinf(D["M"][0]) and np.isneginf(D["M"][1:3]).all() and np.isfinite(D["M"][3])
    assert not D["count"][:3].any() and not D["mass"][:3].any() and (D["best_id"][:3] == -1).all() and np.isneginf(D["best_score"][:3]).all()
    assert (T["label"][:3] == -1).all() and np.isneginf(T["logp"][:3]).all() and (T["n_listed"][:3] == 0).all() and np.isneginf(T["rest_logp"][:3]).all()
    assert np.isneginf(D["lognorm"][:3]).all() and T["n_listed"][3] == 7
    assert_tight({k: v[3:] for k, v in D.items()}, LO.dense(rows[3:], None, lab, 7), "explicit row")
    assert ctx.take_bad_ids() == 0


def test_unlabelled_empty_labels_short_lists_and_emptied_rows(ctx, devs):
    reset(ctx)
    V = devs("geo200")                                                               # "mixed": every seventh POI unlabelled
    C = V.C
    lab = C["labels"]
    D = dense_call(ctx, V, ex=(None, None))
    assert np.array_equal(D["count"][:, V.L], np.full(V.n, (lab < 0).sum())) and (D["mass"][:, V.L] > 0).all()
    empty = [l for l in range(V.L) if not (lab == l).any()]
    assert empty and not D["count"][:, empty].any() and (D["best_id"][:, empty] == -1).all()
    T = topk_call(ctx, V, "mass", 32, ex=(None, None))
    listed = V.L - len(empty)
    assert (T["n_listed"] == min(32, listed)).all() and not np.isin(T["label"], empty + [V.L]).any()
    assert np.isfinite(T["rest_logp"]).all()
    # "five": k above the number of labels - the tail is fill
    F = devs("five")
    T5 = topk_call(ctx, F, "mass", 32)
    assert (T5["n_listed"] == 5).all() and (T5["label"][:, 5:] == -1).all() and np.isneginf(T5["logp"][:, 5:]).all()
    assert (T5["best_id"][:, 5:] == -1).all() and np.isneginf(T5["best_score"][:, 5:]).all()
    assert np.allclose(np.exp(T5["logp"][:, :5]).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # lists that empty a label (row 0: every POI of label 2) or the whole row (row 1), next to an untouched row
    f = F.C["labels"]
    lists = FO.csr([np.nonzero(f == 2)[0], np.arange(F.N), []])
    E = dense_call(ctx, F, rows=[0, 1, 2], ex=lists)
    assert E["count"][0, 2] == 0 and E["mass"][0, 2] == 0 and E["best_id"][0, 2] == -1 and E["count"][0, [0, 1, 3, 4]].all()
    assert not E["count"][1].any() and np.isfinite(E["M"][1]) and np.isneginf(E["lognorm"][1])
    TE = topk_call(ctx, F, "mass", 5, rows=[0, 1, 2], ex=lists)
    assert TE["n_listed"].tolist() == [4, 0, 5] and 2 not in TE["label"][0] and (TE["label"][1] == -1).all() and np.isneginf(TE["logp"][1]).all()
    ref = dense_call(ctx, F, rows=[2], ex=(None, None))
    bits_equal({k: v[2:] for k, v in E.items()}, ref, "the untouched row", DENSE)
    assert ctx.take_bad_ids() == 0


def test_a_half_table(pa, ctx):
    import torch
    reset(ctx)
    C = LC.case("cat37")
    items16 = torch.as_tensor(C["items"]).to(torch.float16).cuda().contiguous()
    ctx.register_f16(items16)
    try:
        V = Dev(C, items=items16)
        _, rows32 = score_rows(ctx, V)
        ref = np.float64(C["users"]) @ np.float64(C["items"].astype(np.float16))[:-1].T
        assert np.abs(rows32 - ref).max() <= RTOL * max(1.0, np.abs(ref).max())       # (the rows are the half table's)
        got = dense_call(ctx, V)
        assert_tight(got, LO.dense(rows32, LC.ex_mask(C), C["labels"], V.L), "half table")
        for by in ("mass", "max"):
            assert_topk_of_dense(topk_call(ctx, V, by, 10), got, by, 10, "half table by %s" % by)
    finally:
        ctx.unregister_f16(items16)


def test_argument_errors_and_bad_rows(ctx, devs):
    reset(ctx)
    V = devs("geo11")
    for k in (0, 33, -1):
        topk_call(ctx, V, "mass", k, expect=ENOTSUP)
    topk_call(ctx, V, 2, 5, expect=EINVAL)
    topk_call(ctx, V, "mass", 5, n_label=0, expect=EINVAL)
    dense_call(ctx, V, n_label=V.N + 1, expect=EINVAL)
    sc = dev(np.zeros((2, 40), np.float32))
    lab = dev(np.zeros(40, np.int32))
    scores_call(ctx, sc, 40, lab, 1, k=33, expect=ENOTSUP)
    scores_call(ctx, sc, 41, lab, 1, expect=EINVAL)                                  # ld < n_item
    assert ctx.lib.poi_score_labels(ctx.handle, p(V.users), p(V.items), 1, 1 << 27, V.dim, None, None, None, None, None, None, 0, 0.0, p(V.labels), 1,
                                    None, None, None, None, None, None, None, None, None) == ENOTSUP
    # malformed lists and anchors: the row is all fill and counted once, its neighbours are untouched
    rows = np.arange(6)
    lists = FO.csr([[], [9, 8, 7], [3, V.N], [5, 5], [], []])
    anchor = V.C["geo"]["anchor"][rows].copy()
    anchor[4] = V.N                                                                  # outside [-1, n_item)
    D = dense_call(ctx, V, rows, ex=lists, anchor=anchor)
    assert ctx.take_bad_ids() == 4
    badr = [1, 2, 3, 4]
    assert not D["count"][badr].any() and not D["mass"][badr].any() and (D["best_id"][badr] == -1).all() and np.isneginf(D["M"][badr]).all()
    T = topk_call(ctx, V, "max", 5, rows, ex=lists, anchor=anchor)
    assert ctx.take_bad_ids() == 4
    assert (T["label"][badr] == -1).all() and np.isneginf(T["logp"][badr]).all() and (T["n_listed"][badr] == 0).all()
    good = dense_call(ctx, V, [0, 5], ex=(None, None))
    bits_equal({k: v[[0, 5]] for k, v in D.items()}, good, "the good rows beside bad ones", DENSE)
    S, _ = scores_call(ctx, dev(np.ones((3, 40), np.float32)), 40, lab, 1, ex=FO.csr([[1, 2], [2, 1], [40]]))
    assert ctx.take_bad_ids() == 2 and S["count"][:, 0].tolist() == [38, 0, 0]


# ---- 5: every model class, both session kinds, the evaluation -----------------------------------------------------------------------------
def check_model_rows(out, full, mask, lab, n_label, by, k, what, same_rows=False):
    """recommend_labels(..., return_best=True) against the oracle on the model's own float32 score rows: the lists on the clear rows
    (at least 90 %), log p to RTOL.  same_rows: the kernel reads exactly these float32 rows (the explicit-rows entry), so a row is clear
    as soon as the masses differ by more than the exp routines can (labels_oracle.clear_rows_tight); otherwise the rows are summed in
    another order than the walk's product and the float64 margin decides."""
    got = [t.cpu().numpy() for t in out]
    D = LO.dense(full, mask, lab, n_label)
    W = LO.topk(D, by, k)
    clear = LO.clear_rows_tight(D, by, k) if same_rows else LO.clear_rows(D, full, by, k)
    print("%s by %s: %.0f %% of %d rows clear" % (what, by, 100 * clear.mean(), len(clear)))
    assert clear.mean() >= 0.9, what
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(got[0][clear], W["label"][clear]) and np.array_equal(got[2][clear], W["best_id"][clear]), what
    fin = clear[:, None] & np.isfinite(W["logp"])
    tol = RTOL * max(1.0, float(np.abs(np.where(np.isfinite(full), full, 0)).max()))
    assert np.abs(got[1][fin] - W["logp"][fin]).max(initial=0) <= tol and np.abs(got[3][fin] - W["best_score"][fin]).max(initial=0) <= tol, what
    assert np.array_equal(got[0] >= 0, W["label"] >= 0), what
    return D


@pytest.mark.parametrize("cls", ["bpr", "spatial", "gru", "vbpr", "fpmc", "geoie", "lstm", "rnn"])
def test_every_fused_class_against_the_oracle_on_its_own_score_rows(pa, ctx, cls):
    from tests.test_gpu_capped import fused_model
    reset(ctx)
    if cls in ("bpr", "spatial"):
        from tests.test_gpu_near import make_case
        m, users = make_case(cls, 32, 640, n_user=70, n_item=300)["build"](pa), np.arange(70)
    else:
        m, users = fused_model(pa, cls)
    assert m._rank_fused, cls
    n, N = len(users), m.n_item
    full = m.compute_sub_all_scores_device(users).cpu().numpy()
    lab = (np.arange(N) * 7 % 6).astype(np.int32)
    lab[::9] = -1
    labels = m.poi_labels(lab)
    lists = FO.csr([np.sort(np.random.default_rng(r).choice(N, r % 20, replace=False)) for r in range(n)])
    mask, _ = FO.candidate_masks(np.ones((1, N), bool), None, n, *lists)
    for by in ("mass", "max"):
        D = check_model_rows(m.recommend_labels(users, 4, labels, by=by, exclude=lists, return_best=True), full, mask, lab, 6, by, 4, cls)
    out = m.recommend_labels(users, 4, labels)
    assert isinstance(out, tuple) and len(out) == 2 and out[0].shape == (n, 4)
    prob, rest = (t.cpu().numpy() for t in m.label_distribution(users, labels, exclude=lists))
    want = LO.f64(D["mass"]) / LO.f64(D["total"])[:, None]
    assert prob.shape == (n, 6) and prob.dtype == np.float64 and np.abs(prob - want[:, :6]).max() <= RTOL and np.abs(rest - want[:, 6]).max() <= RTOL
    assert np.allclose(prob.sum(axis=1) + rest, 1.0, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        m.recommend_labels(users, 33, labels)
    with pytest.raises(ValueError):
        m.recommend_labels(users, 4, labels, by="sum")
    with pytest.raises(IndexError, match="1 row"):
        m.recommend_labels(users[:3], 4, labels, exclude=(dev(np.array([0, 2, 2, 2], np.int32)), dev(np.array([7, 3], np.int32))))
    assert ctx.take_bad_ids() == 0


def test_own_rule_models_go_through_their_own_score_rows(pa, ctx):
    from tests.test_gpu_capped import own_rule_models
    reset(ctx)
    for name, m, users in own_rule_models(pa):
        assert not m._rank_fused, name
        n, N = len(users), m.n_item
        full = m._own_score_rows(users)(0, n).cpu().numpy()
        lab = (np.arange(N) * 7 % 5).astype(np.int32)
        lab[::9] = -1
        labels = m.poi_labels(lab)
        lists = FO.csr([np.sort(np.random.default_rng(r).choice(N, r % 20, replace=False)) for r in range(n)])
        mask, _ = FO.candidate_masks(np.ones((1, N), bool), None, n, *lists)
        for by in ("mass", "max"):
            D = check_model_rows(m.recommend_labels(users, 3, labels, by=by, exclude=lists, return_best=True), full, mask, lab, 5, by, 3, name, same_rows=True)
        got = [t.cpu().numpy() for t in m.recommend_labels(users, 5, labels, by="max", exclude=lists, return_best=True)]
        W = LO.topk(D, "max", 5)                                                      # the same float32 rows: by max is exact on every row
        assert np.array_equal(got[0], W["label"]) and np.array_equal(got[2], W["best_id"]) and same_bits(got[3], W["best_score"]), name
        prob, rest = (t.cpu().numpy() for t in m.label_distribution(users, labels, exclude=lists))
        want = LO.f64(D["mass"]) / LO.f64(D["total"])[:, None]
        assert np.abs(prob - want[:, :5]).max() <= RTOL and np.abs(rest - want[:, 5]).max() <= RTOL, name


@pytest.mark.parametrize("kind", ["spatial", "lstm", "carnn"])
def test_session_recommend_labels_is_the_oracle_on_the_sessions_scores(pa, kind):
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
    lab = (np.arange(300) * 7 % 6).astype(np.int32)
    lab[::11] = -1
    labels = m.poi_labels(lab)
    lists = FO.csr([np.sort(np.random.default_rng(r).choice(300, r % 40, replace=False)) for r in range(T["n_user"])])
    mask, _ = FO.candidate_masks(np.ones((1, 300), bool), None, T["n_user"], *lists)
    if kind == "carnn":
        n, rows_of, has, _ = s._carnn_rows(slots)
        full = rows_of(0, n).cpu().numpy()
        full[~has.cpu().numpy()] = -np.inf
    else:
        ids, sc = (t.cpu().numpy() for t in s.candidates(slots, 300, return_scores=True))
        full = np.full((T["n_user"], 300), -np.inf, np.float32)
        np.put_along_axis(full, ids, sc, 1)
    for by in ("mass", "max"):
        out = s.recommend_labels(slots, 4, labels, by=by, exclude=dev_ex(lists), return_best=True)
        check_model_rows(out, full, mask, lab, 6, by, 4, "%s session" % kind, same_rows=kind == "carnn")
    if kind == "carnn":                                  # a slot without a check-in: nothing scorable, all fill
        got = [t.cpu().numpy() for t in out]
        assert (got[0][-2:] == -1).all() and np.isneginf(got[1][-2:]).all()
    with pytest.raises(ValueError):
        s.recommend_labels(slots, 4, labels, exclude="train")
    with pytest.raises(ValueError):
        s.recommend_labels(slots, 0, labels)


def test_label_hit_rate_on_a_tiny_trained_model(pa, ctx):
    """evaluate.label_hit_rate against a host count from recommend_labels' own lists, by mass beside by max, on a BPR model trained for
    a few epochs on a synthetic data set whose users stay inside their home categories."""
    from poi_amd import evaluate as E
    rng = np.random.default_rng(5)
    n_user, n_item, n_cat, L = 96, 400, 8, 10
    cat = rng.integers(0, n_cat, n_item)
    home = rng.integers(0, n_cat, n_user)
    seqs = [rng.choice(np.nonzero(cat == home[u])[0], L) if rng.random() < 0.9 else rng.integers(0, n_item, L) for u in range(n_user)]
    P = np.array(seqs)
    train = [P[:, :-1], np.ones((n_user, L - 1), int), rng.integers(0, n_item, (n_user, L - 1))]
    test = [P[:, -1:], np.ones((n_user, 1), int), rng.integers(0, n_item, (n_user, 1))]
    m = pa.models.OboBpr(train=train, test=test, alpha_lambda=[0.05, 0.001], n_user=n_user, n_item=n_item, n_in=16, n_hidden=16)
    u, pp = np.repeat(np.arange(n_user), L - 1), P[:, :-1].reshape(-1)
    for _ in range(300):
        qq = rng.integers(0, n_item, len(u))
        m.train_batch(u, pp, np.where(qq == pp, (qq + 1) % n_item, qq))
    m.update_trained_items(); m.update_trained_users()
    labels = m.poi_labels(cat.astype(np.int32), n_cat)
    ks = [1, 2, 4]
    se = [np.arange(0, 50), np.arange(50, n_user)]      # batches of user ids, as the drivers' starts_ends_tes
    rates = {by: E.label_hit_rate(m, labels, se, ks, by) for by in ("mass", "max")}
    print("label hit rate by mass %s, by max %s" % (rates["mass"], rates["max"]))
    for by in ("mass", "max"):
        top = m.recommend_labels(np.arange(n_user), 4, labels, by=by)[0].cpu().numpy()
        want = cat[P[:, -1]]
        for k in ks:
            assert rates[by][k] == pytest.approx(float((top[:, :k] == want[:, None]).any(axis=1).mean()), abs=1e-12), (by, k)
        assert 0.0 <= rates[by][1] <= rates[by][2] <= rates[by][4] <= 1.0
    assert rates["mass"][1] > 1.0 / n_cat                # the trained model beats a uniform guess at the category
    with pytest.raises(ValueError):
        E.label_hit_rate(m, labels, se, [2, 1], "mass")
