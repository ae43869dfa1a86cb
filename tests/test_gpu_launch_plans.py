"""-m gpu: the training step against the float64 oracle at every launch size where its plan switches.  poi_spatial_step / poi_gru_step pick
among a dozen kernel plans from the launch size n and the table shape (abi.hip te_setup / seq_step, te_scatter.hip): the one-sequence path,
the touched-row list of the write-back ("listed"), the float64 per-sequence forward (xrec1), the HYBRID recurrences (per-sequence kernels
and 16-sequence tiles at the same time, dim 128, the split chosen on the device), the per-bin tables and per-POI regrouping (bintab / ppoi),
the compact exact-forward table (xcomp), the per-sequence backward (rec1) and the forked write-back.  The other suites check the step at
toy launches (<= 160 sequences) and at the 12500-sequence timed launch only; this file checks every plan in between, with the DEFAULT
context options (a context of its own: nothing an earlier test set carries over), in bench.py's configuration (Gowalla shape, 80 % local
transitions, batch cap 64, launches sorted by length):
  * losses, all nine tensors to 1e-5 and every row's update to 1e-4 of its own absolute mass (tests/gpu_util), every lt row inside 1e-5,
    and the rows that move == the rows the oracle's launch touches;
  * the same launch twice from identical tables: tables and losses bitwise equal, and the same plan;
  * the plan itself (poi_ctx_last_plan): each documented threshold is asserted on both sides, so a retuned constant fails here loudly
    instead of quietly moving what the suite covers.
Printed: one line per launch with its plan flags, the hybrid split and the worst delta excess (<= 1 passes)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SP_NAMES = ("lt", "di", "ui", "wh", "bi", "vs", "bs", "wd", "loss_weight")
GRU_NAMES = ("lt", "ui", "wh", "bi")
FLAGS = ("tile", "one", "listed", "xrec1", "rec1", "hyb", "bintab", "ppoi", "xft", "xcomp", "fwd_tab", "head_split", "efuse", "early_bins", "fork")
CAP = 64.0                 # bench.py --batch-cap
ALPHA, LAMBDA = 0.01, 0.001
# the context defaults (abi.hip struct poi_ctx) this file pins
HYB_MIN, HYB_MAX, XREC1_MAX, REC1_MAX, BINTAB_MIN, XCOMP_MIN, EARLY_MIN = 1150, 2300, 1100, 1800, 1280, 1536, 1024
SIZES = [1, 2, 17, 256, 1100, 1101, 1149, 1150, 1279, 1280, 1535, 1536, 1563, 1800, 1801, 2047, 2048, 2300, 2301, 4096]


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16), os.cpu_count() or 1))


def listed_max(n_item, n_dist, max_len):
    """Largest launch whose write-back keeps a touched-row list: abi.hip te_setup, `listed = Rrows > 4 * Ncap` with
    Ncap = 3 (Tcap + n), Tcap = n (max_len - 1) + 192."""
    R = n_item + 1 + n_dist + 1
    n = 0
    while R > 4 * 3 * ((n + 1) * (max_len - 1 if max_len > 1 else 1) + 192 + (n + 1)):
        n += 1
    return n


def expected_plan(n, dim, spatial, n_item, n_dist, max_len):
    """The plan the defaults document (abi.hip struct poi_ctx and te_setup) for a training launch of n sequences."""
    Tcap = n * (max_len - 1 if max_len > 1 else 1) + 192
    hyb = int(dim == 128 and HYB_MIN <= n <= HYB_MAX and n > 1)
    bintab = int(spatial and dim >= 128 and n >= BINTAB_MIN)
    want_ft = 2 * (n_item + 1) <= Tcap
    want_xc = bool(bintab and n >= XCOMP_MIN)
    return dict(tile=1, one=int(n == 1), listed=int(n <= listed_max(n_item, n_dist if spatial else -1, max_len)),
                xrec1=int(n <= XREC1_MAX and not hyb), rec1=int(n <= REC1_MAX and not hyb), hyb=hyb, bintab=bintab, ppoi=bintab,
                xft=int((want_ft or want_xc) and n > 1), xcomp=int(want_xc), fwd_tab=0, early_bins=int(bintab and n >= EARLY_MIN), fork=0)


def _check_plan(plan, n, dim, spatial, n_item, n_dist, max_len):
    exp = expected_plan(n, dim, spatial, n_item, n_dist, max_len)
    bad = {k: (plan[k], v) for k, v in exp.items() if plan[k] != v}
    assert not bad, "n = %d: plan flags (got, documented) %s" % (n, bad)
    if plan["hyb"]:
        for k in ("fwd", "bwd"):
            s, wg = plan["hyb_%s_seq" % k], plan["hyb_%s_wg" % k]
            assert 0 <= s <= n and wg >= 1, (n, k, s, wg)
    else:
        assert all(plan["hyb_%s" % k] == -1 for k in ("fwd_seq", "fwd_wg", "bwd_seq", "bwd_wg"))


class Bench:
    """One model on its own context with the default options; every launch starts from the same (fresh-model) tables."""

    def __init__(self, pa, ds, tab, make, names):
        import torch
        self.pa, self.ds, self.tab, self.names = pa, ds, tab, names
        self.ctx = pa._lib.Context(0)
        self.m = make()
        self.m.ctx = self.ctx
        self.init = [getattr(self.m, k).t.clone() for k in names]
        self.P = {k: (float(v) if k == "wd" else np.asarray(v, np.float64)) for k, v in ((k, getattr(self.m, k).get_value()) for k in names)}
        self.P["h0"] = np.zeros(self.P["lt"].shape[1])
        self.lens = np.diff(tab.off.astype(np.int64))
        torch.cuda.synchronize()

    def users(self, n, order="sorted"):
        u = np.random.default_rng(5).permutation(self.ds.n_user)[:n].astype(np.int32)
        return u[np.argsort(-self.lens[u], kind="stable")] if order == "sorted" else u

    def launch(self, users, cap):
        """-> (out, device tensors after the launch, plan)"""
        import torch
        for t, t0 in zip((getattr(self.m, k).t for k in self.names), self.init):
            t.copy_(t0)
        self.ctx.set_batch_cap(cap)
        try:
            out = np.asarray(self.m.train_batch(users))
        finally:
            self.ctx.set_batch_cap(1.0)
        plan = self.ctx.last_plan()
        torch.cuda.synchronize()
        return out, [getattr(self.m, k).t.clone() for k in self.names], plan

    def state(self):
        return {k: (float(v) if k == "wd" else np.asarray(v, np.float64)) for k, v in ((k, getattr(self.m, k).get_value()) for k in self.names)}

    def close(self):
        self.m.ctx = self.pa._lib.context(0)
        self.ctx.close()


def _bitwise_equal(a, b):
    import torch
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _spatial_bench(shape, seed, model_seed):
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    from poi_amd import data as pdata
    n_item, n_user, max_len, D = pdata.SHAPES[shape]
    ds = pdata.make_synthetic(n_user, n_item, max_len, seed=seed, local=0.8)      # bench.py's generator setting (--local 0.8)
    tab = ds.shard(0, n_user)

    def make():
        return poi_amd.models.OboSpatialGru(train=tab, test=None, dist=None, alpha_lambda=[ALPHA, LAMBDA], n_user=n_user, n_item=n_item,
                                            n_dists=[ds.dist_num, ds.dd / 1000.0], n_in=D, n_hidden=D, seed=model_seed, coords=ds.coords)
    return Bench(poi_amd, ds, tab, make, SP_NAMES)


@pytest.fixture(scope="module")
def gowalla():
    b = _spatial_bench("gowalla", 77, 3)           # test_gpu_fullsize.py's data
    assert b.ds.dist_num == 200 and b.P["lt"].shape[1] == 128
    yield b
    b.close()


_ORACLE = {}
_PLANS = {}


def _oracle(b, n, cap, keep=False):
    """The C oracle's batch rule for the sorted n-sequence launch of bench `b`: (users, P_new, out, touched); cached per (size, cap)
    only when `keep` (a Gowalla-size result is ~0.3 GB)."""
    from oracle import c_oracle as C
    key = (id(b), n, cap)
    if key in _ORACLE:
        return _ORACLE[key]
    users = b.users(n)
    t = b.tab
    exp, eout, touched = C.spatial_batch_mean(b.P, t.off, t.p, t.q, t.dp, t.dq, users, t.len_max, ALPHA, LAMBDA, threads=_threads(),
                                              cap=cap, absmass=True)
    res = (users, exp, eout, touched)
    if keep:
        _ORACLE[key] = res
    return res


def _run_and_check(b, n, cap, order="sorted", what="", keep=False):
    """One launch against the oracle + the bitwise rerun; returns (plan, worst delta excess)."""
    from tests.gpu_util import assert_close, assert_step_close, delta_excess, rows_within
    users0, exp, eout, touched = _oracle(b, n, cap, keep=keep)
    users = users0 if order == "sorted" else b.users(n, order)
    out, tabs, plan = b.launch(users, cap)
    got = b.state()
    out2, tabs2, plan2 = b.launch(users, cap)
    tag = "%s n = %d (%s, cap %g)" % (what, n, order, cap)
    assert plan2 == plan, (tag, plan, plan2)
    assert _bitwise_equal(tabs, tabs2), "%s: tables differ between identical launches" % tag
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "%s: losses differ between identical launches" % tag
    pos = {int(u): i for i, u in enumerate(users0)}
    eo = eout[[pos[int(u)] for u in users]]
    assert_close(out[:, :3], eo[:, :3], "losses " + tag)
    assert_step_close(got, exp, b.P, b.names, tag, absmass=touched["absmass"])
    assert rows_within(got["lt"], exp["lt"]) == 1.0, "%s: POI rows miss the 1e-5 bar" % tag
    assert np.array_equal((got["lt"] != b.P["lt"]).any(axis=1), touched["lt"]), "%s: rows changed != rows the oracle touches" % tag
    worst = max(delta_excess(got[k], exp[k], b.P[k], absmass=touched["absmass"][k])[0] for k in b.names)
    return plan, worst


def _line(n, order, cap, plan, worst):
    fl = " ".join("%s=%d" % (k, plan[k]) for k in FLAGS if k != "tile")
    split = "fwd %d seq / %d wg, bwd %d seq / %d wg" % (plan["hyb_fwd_seq"], plan["hyb_fwd_wg"], plan["hyb_bwd_seq"], plan["hyb_bwd_wg"]) if plan["hyb"] else "-"
    print("[plan] n %5d %-6s cap %3g | %s | hybrid split: %s | worst delta excess %.3f" % (n, order, cap, fl, split, worst))


CASES = [(n, "sorted") for n in SIZES] + [(1563, "caller")]


def _sizes_with_listed(b):
    L = listed_max(b.ds.n_item, b.ds.dist_num, int(b.lens.max()))
    return L, [L - 1, L, L + 1, L + 2]


@pytest.mark.parametrize("n,order", CASES, ids=["%d-%s" % c for c in CASES])
def test_spatial_launch_matches_the_oracle_and_its_documented_plan(gowalla, n, order):
    b = gowalla
    plan, worst = _run_and_check(b, n, CAP, order, "gowalla", keep=(n == 1563 or n == 2048))
    _line(n, order, CAP, plan, worst)
    _PLANS[("gowalla", n, order)] = plan
    _check_plan(plan, n, 128, True, b.ds.n_item, b.ds.dist_num, int(b.lens.max()))
    if n == 1563 and order == "sorted":      # the 8-GPU schedule's launch: the device must really split it between the two kernels
        assert plan["hyb"] == 1
        assert 0 < plan["hyb_fwd_seq"] < n and 0 < plan["hyb_bwd_seq"] < n, plan


def test_spatial_launches_around_the_listed_boundary(gowalla):
    b = gowalla
    L, sizes = _sizes_with_listed(b)
    assert 17 < L < 256, L                   # (between the sweep's sizes: roughly 160 at the Gowalla shape)
    for n in sizes:
        plan, worst = _run_and_check(b, n, CAP, "sorted", "gowalla")
        _line(n, "sorted", CAP, plan, worst)
        _PLANS[("gowalla", n, "sorted")] = plan
        _check_plan(plan, n, 128, True, b.ds.n_item, b.ds.dist_num, int(b.lens.max()))


def _plan_of(b, n, tag):
    if (tag, n, "sorted") not in _PLANS:
        _PLANS[(tag, n, "sorted")] = b.launch(b.users(n), CAP)[2]
    return _PLANS[(tag, n, "sorted")]


def test_each_threshold_flips_its_flag_between_the_two_sizes(gowalla):
    """For every documented switch: the named flag differs between the last size below and the first size above it."""
    b = gowalla
    L, _ = _sizes_with_listed(b)
    pairs = [(1, 2, "one", 1), (L, L + 1, "listed", 1), (1100, 1101, "xrec1", 1), (1149, 1150, "hyb", 0), (1149, 1150, "rec1", 1),
             (2300, 2301, "hyb", 1), (1279, 1280, "bintab", 0), (1279, 1280, "ppoi", 0), (1535, 1536, "xcomp", 0)]
    for lo, hi, flag, below in pairs:
        a, c = _plan_of(b, lo, "gowalla")[flag], _plan_of(b, hi, "gowalla")[flag]
        assert (a, c) == (below, 1 - below), "%s: n = %d -> %d, n = %d -> %d (expected %d -> %d)" % (flag, lo, a, hi, c, below, 1 - below)
    # the forked write-back (te_scatter.hip, >= 2048 sequences) is unreachable with the default options: every launch large enough for
    # it has the early distance-bin chain (early_min 1024 < bintab_min 1280), which it excludes - covered with early_bins off below
    assert _plan_of(b, 2047, "gowalla")["fork"] == 0 and _plan_of(b, 2048, "gowalla")["fork"] == 0
    for n in (1150, 1563, 2048, 2300):
        p = _plan_of(b, n, "gowalla")
        print("[split] n %d: forward %d sequences on %d workgroups, backward %d on %d" % (n, p["hyb_fwd_seq"], p["hyb_fwd_wg"], p["hyb_bwd_seq"], p["hyb_bwd_wg"]))


def test_forked_write_back_matches_the_oracle(gowalla):
    """early_bins off (option "early_bins"): the 2048-sequence launch forks the distance-bin chain of its write-back onto the side stream."""
    b = gowalla
    b.ctx.set_option("early_bins", 0)
    try:
        plan, worst = _run_and_check(b, 2048, CAP, "sorted", "gowalla early_bins=0", keep=True)
        _line(2048, "fork", CAP, plan, worst)
        assert plan["fork"] == 1 and plan["early_bins"] == 0 and plan["bintab"] == 1, plan
        plan2 = b.launch(b.users(2047), CAP)[2]
        assert plan2["fork"] == 0 and plan2["early_bins"] == 0, plan2
    finally:
        b.ctx.set_option("early_bins", 1)


@pytest.mark.parametrize("n", [1150, 2048])
def test_spatial_launch_cap_1_matches_the_mean_rule(gowalla, n):
    b = gowalla
    plan, worst = _run_and_check(b, n, 1.0, "sorted", "gowalla mean rule")
    _line(n, "sorted", 1.0, plan, worst)
    _check_plan(plan, n, 128, True, b.ds.n_item, b.ds.dist_num, int(b.lens.max()))


def test_graph_replay_records_the_plan_of_the_launch_it_replays(gowalla):
    """A replayed launch (poi_ctx_set_graph) reports the eager launch's plan, the device's hybrid split included."""
    b = gowalla
    users = b.users(1563)
    eager = b.launch(users, CAP)
    b.ctx.set_graph(True)
    try:
        runs = [b.launch(users, CAP) for _ in range(3)]          # eager (first sight), capture + replay, replay
        assert b.ctx.graph_replays() >= 2
    finally:
        b.ctx.set_graph(False)
    for out, tabs, plan in runs:
        assert plan == eager[2], (plan, eager[2])
        assert _bitwise_equal(tabs, eager[1]) and np.array_equal(out.view(np.uint32), eager[0].view(np.uint32))


# ---- dim 64 (Foursquare shape): the hybrid is off, the per-sequence thresholds are the same ------------------------------------------------
@pytest.fixture(scope="module")
def foursquare():
    b = _spatial_bench("foursquare", 78, 4)        # test_gpu_fullsize.py's data
    assert b.P["lt"].shape[1] == 64
    yield b
    b.close()


@pytest.mark.parametrize("lo,hi,flag", [(1100, 1101, "xrec1"), (1800, 1801, "rec1"), (2047, 2048, None)])
def test_dim64_launches_match_the_oracle_without_the_hybrid(foursquare, lo, hi, flag):
    b = foursquare
    plans = []
    for n in (lo, hi):
        plan, worst = _run_and_check(b, n, CAP, "sorted", "foursquare")
        _line(n, "d64", CAP, plan, worst)
        assert plan["hyb"] == 0 and plan["hyb_fwd_seq"] == -1
        _check_plan(plan, n, 64, True, b.ds.n_item, b.ds.dist_num, int(b.lens.max()))
        plans.append(plan)
    if flag:
        assert (plans[0][flag], plans[1][flag]) == (1, 0), (flag, plans)


# ---- plain GRU (poi_gru_step): the hybrid predicate has no spatial condition ----------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    from poi_amd import data as pdata
    n_item, n_user, max_len, D = 3000, 4000, 20, 128
    ds = pdata.make_synthetic(n_user, n_item, max_len, seed=79, local=0.8)
    tab = ds.shard(0, n_user)

    def make():
        return poi_amd.models.OboGru(train=tab, test=None, alpha_lambda=[ALPHA, LAMBDA], n_user=n_user, n_item=n_item, n_in=D, n_hidden=D, seed=5)
    b = Bench(poi_amd, ds, tab, make, GRU_NAMES)
    b.padded = ds.to_padded()["train"]           # [pois, mask, negatives] in the reference's padded layout (pad = n_item)
    yield b
    b.close()


def _gru_oracle(b, users):
    """tests/gpu_util.batch_mean_update over oracle.poi_oracle.gru_step, accumulated one sequence at a time (holding every sequence's
    whole new table would take gigabytes): each row moves by the mean of the updates of the sequences touching it, dense tensors by the
    mean over the launch."""
    from oracle import poi_oracle as O
    Pm, Mm, Qm = b.padded
    P = b.P
    acc = {k: np.zeros_like(P[k]) for k in GRU_NAMES}
    cnt = np.zeros(P["lt"].shape[0])
    losses = np.empty(len(users))
    for i, u in enumerate(users):
        Pn, losses[i] = O.gru_step(P, Pm[u], Qm[u], Mm[u], ALPHA, LAMBDA)
        R = np.unique(np.concatenate((Pm[u], Qm[u])))
        acc["lt"][R] += Pn["lt"][R] - P["lt"][R]
        cnt[R] += 1
        for k in ("ui", "wh", "bi"):
            acc[k] += Pn[k] - P[k]
    exp = {k: P[k] + acc[k] / len(users) for k in ("ui", "wh", "bi")}
    nz = cnt > 0
    exp["lt"] = P["lt"].copy()
    exp["lt"][nz] += acc["lt"][nz] / cnt[nz, None]
    return exp, losses, nz


@pytest.mark.parametrize("n", [1150, 1563])
def test_plain_gru_hybrid_launch_matches_the_mean_rule(plain, n):
    from tests.gpu_util import assert_close, assert_step_close, delta_excess
    b = plain
    users = b.users(n)
    exp, losses, touched = _gru_oracle(b, users)
    out, tabs, plan = b.launch(users, 1.0)
    got = b.state()
    out2, tabs2, plan2 = b.launch(users, 1.0)
    assert plan2 == plan and _bitwise_equal(tabs, tabs2) and np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    assert_close(out.reshape(-1), losses, "plain GRU losses n = %d" % n, rtol=2e-5)
    assert_step_close(got, exp, b.P, GRU_NAMES, "plain GRU n = %d" % n)
    assert np.array_equal((got["lt"] != b.P["lt"]).any(axis=1), touched)
    worst = max(delta_excess(got[k], exp[k], b.P[k])[0] for k in GRU_NAMES)
    _line(n, "gru", 1.0, plan, worst)
    _check_plan(plan, n, 128, False, b.ds.n_item, -1, int(b.lens.max()))
    assert plan["hyb"] == 1 and plan["bintab"] == 0
