"""-m gpu tests of the leave-one-out attribution (models.Explainer.explain -> poi_explain_loo): base and delta must equal the float64
oracle's `predict` on every reduced history (tests/explain_oracle.py) at the project's RTOL - delta relative to max|oracle delta| - with
the keys and offsets exact.  The identities of the code's own paths (start mode, batching, order) are bitwise; the comparison with
the route that existed before (a Session replayed through the reduced histories + score_lists) is at RTOL."""
import numpy as np
import pytest

from tests import explain_oracle as XO
from tests.gpu_util import RTOL, assert_close
from tests.test_gpu_session import geo_problem, gru_init, plain_model, seqs_of, spatial_init, spatial_model

pytestmark = pytest.mark.gpu

C = 20


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def explainer(m):
    from poi_amd import models
    return models.Explainer(m)


def make_lists(seed, n, n_item, holes=(3, 11)):
    """(n, C) random POIs with two -1 entries per row."""
    lists = np.random.default_rng(seed).integers(0, n_item, (n, C))
    for h in holes:
        lists[:, h] = -1
    return lists


def csr(seqs):
    off = np.r_[0, np.cumsum([len(s) for s in seqs])].astype(np.int64)
    flat = np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in seqs]) if off[-1] else np.zeros(0, np.int64)
    return off, flat


def run(m, seqs, lists, **kw):
    """explain() on explicit histories -> host arrays."""
    out = explainer(m).explain(np.zeros(len(seqs), np.int64), lists, histories=csr(seqs), **kw)
    host = [o.cpu().numpy() if hasattr(o, "cpu") else o for o in out]
    if kw.get("return_states"):
        host[4] = {k: v.cpu().numpy() for k, v in out[4].items()}
    return host


def check_against_oracle(got, R, what):
    base, delta, off, keys = got[:4]
    assert np.array_equal(off, R["off"]) and np.array_equal(keys, R["keys"]), what
    for name, a, b in (("base", base, R["base"]), ("delta", delta, R["delta"])):
        assert a.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b)), (what, name)
        e = assert_close(np.nan_to_num(a), np.nan_to_num(b), "%s %s" % (what, name)) if b.size else 0.0
        print("%s: %s max|hip - oracle| / max|oracle| = %.2e (max|oracle| %.3g)" % (what, name, e, np.abs(np.nan_to_num(b)).max() if b.size else 0.0))


# ---- 1: spatial, with an empty history; the re-binning is exercised ------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 8])
def test_spatial_equals_the_oracle_and_rebins(pa, dim):
    T = geo_problem(101, n_user=24, n_item=50, n_dist=11, dim=dim, len_min=1, len_max=12)
    P = spatial_init(101, T)
    m = spatial_model(pa, T, P)
    assert m.kdim == 64
    seqs = seqs_of(T) + [np.zeros(0, np.int64)]
    lists = make_lists(1, len(seqs), T["n_item"])
    R = XO.explain(P, T, seqs, lists)
    changed, cases = XO.rebinned(T, seqs)
    print("removing a middle check-in changes the next step's bin in %d of %d cases" % (changed, cases))
    assert cases >= 100 and 2 * changed >= cases
    last_rows = [R["off"][r + 1] - 1 for r, s in enumerate(seqs) if len(s) >= 2]      # "remove the last check-in" of every row that keeps one
    rows = [r for r, s in enumerate(seqs) if len(s) >= 2]
    geo_moved = np.nan_to_num(R["base_geo"][rows] - R["var_geo"][last_rows])
    assert np.abs(geo_moved).max() > 0.0, "removing the last check-in must move the distance term of some listed POI"
    got = run(m, seqs, lists)
    assert np.isnan(got[0][:, [3, 11]]).all() and np.isnan(got[1][:, [3, 11]]).all() and not np.isnan(np.delete(got[0], [3, 11], axis=1)).any()
    assert got[2][-1] - got[2][-2] == 0 and len(got[1]) == sum(len(s) for s in seqs)         # the empty history: a base row, no variant
    check_against_oracle(got, R, "spatial dim %d" % dim)


# ---- 2: saturated regime, histories across one, two and three checkpoints -----------------------------------------------------------------
@pytest.fixture(scope="module")
def saturated(pa):
    T = geo_problem(102, n_user=40, n_item=300, n_dist=200, dim=128, len_min=20, len_max=50)
    P = spatial_init(102, T, bias=False)
    return T, P, spatial_model(pa, T, P)


def test_saturated_regime(saturated):
    T, P, m = saturated
    seqs = seqs_of(T)[:8]
    assert min(len(s) for s in seqs) > 16 and max(len(s) for s in seqs) > 48
    lists = make_lists(2, 8, T["n_item"])
    check_against_oracle(run(m, seqs, lists), XO.explain(P, T, seqs, lists), "saturated")
    assert m.ctx.last_plan("explain_columns") == 8 + sum(len(s) for s in seqs) and m.ctx.last_plan("explain_start") == 1


# ---- 3: short histories pack several rows per tile ------------------------------------------------------------------------------------------
def test_packing(pa):
    T = geo_problem(103, n_user=70, n_item=80, n_dist=11, dim=64, len_min=1, len_max=3)
    P = spatial_init(103, T)
    m = spatial_model(pa, T, P)
    seqs = seqs_of(T)
    lists = make_lists(3, 70, T["n_item"])
    R = XO.explain(P, T, seqs, lists)
    assert len(R["delta"]) == 128
    check_against_oracle(run(m, seqs, lists), R, "packing")
    assert m.ctx.last_plan("explain_tiles") == 5 + 8


# ---- 4: the plain models and a half table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["OboGru", "Gru"])
def test_plain_models(pa, cls):
    T = geo_problem(104, n_user=24, n_item=50, n_dist=11, dim=64, len_min=1, len_max=20)
    P = gru_init(104, T)
    m = plain_model(pa, T, P, cls)
    seqs = seqs_of(T)
    lists = make_lists(4, 24, T["n_item"])
    check_against_oracle(run(m, seqs, lists), XO.explain(P, T, seqs, lists, spatial=False), cls)


def test_half_table(pa):
    T = geo_problem(105, n_user=24, n_item=50, n_dist=11, dim=64, len_min=1, len_max=20)
    P = spatial_init(105, T)
    P["lt"] = P["lt"].astype(np.float16).astype(np.float64)            # the oracle runs from the half-rounded table
    m = spatial_model(pa, T, P, table_dtype="f16")
    seqs = seqs_of(T)
    lists = make_lists(5, 24, T["n_item"])
    check_against_oracle(run(m, seqs, lists), XO.explain(P, T, seqs, lists), "half table")


# ---- 5: by="poi" ------------------------------------------------------------------------------------------------------------------------------
def test_by_poi_removes_every_visit(pa):
    T = geo_problem(106, n_user=24, n_item=50, n_dist=11, dim=64, len_min=6, len_max=20)
    P = spatial_init(106, T)
    m = spatial_model(pa, T, P)
    seqs = [np.array(s) for s in seqs_of(T)]
    for u in (0, 5):
        seqs[u][3] = seqs[u][1]                                    # a repeat with a visit between
    for u in (2, 7):
        seqs[u][4] = seqs[u][3]                                    # a consecutive repeat
    lists = make_lists(6, 24, T["n_item"])
    R = XO.explain(P, T, seqs, lists, by="poi")
    assert len(R["delta"]) < sum(len(s) for s in seqs)
    for r, s in enumerate(seqs):
        first = list(dict.fromkeys(int(v) for v in s))
        assert list(R["keys"][R["off"][r]:R["off"][r + 1]]) == first
    check_against_oracle(run(m, seqs, lists, by="poi"), R, "by poi")


# ---- 6: identities of the code's own paths, bitwise -----------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_identities_are_bitwise(saturated):
    T, P, m = saturated
    seqs = seqs_of(T)[:20]
    lists = make_lists(7, 20, T["n_item"])
    ref = run(m, seqs, lists, return_states=True)
    again = run(m, seqs, lists, return_states=True)
    m.ctx.set_option("explain_start", 0)
    try:
        zero = run(m, seqs, lists, return_states=True)
        assert m.ctx.last_plan("explain_start") == 0
    finally:
        m.ctx.set_option("explain_start", 1)
    from poi_amd.models import Explainer
    ws = Explainer.EXPLAIN_WS_BYTES
    Explainer.EXPLAIN_WS_BYTES = 3 * 3 * 128 * 8                               # the checkpoints of three rows at a time: seven chunks
    try:
        chunked = run(m, seqs, lists, return_states=True)
        assert m.ctx.last_plan("explain_columns") == 2 + len(seqs[18]) + len(seqs[19])      # (the last chunk's)
    finally:
        Explainer.EXPLAIN_WS_BYTES = ws
    for name, other in (("two identical calls", again), ("explain_start 0", zero), ("seven chunks", chunked)):
        assert same_bits(ref[0], other[0]) and same_bits(ref[1], other[1]), name
        assert all(same_bits(ref[4][k].astype(np.float64), other[4][k].astype(np.float64)) for k in ref[4]), name
    off = ref[2]
    for r in (0, 7, 19):                                               # a row alone
        one = run(m, [seqs[r]], lists[r:r + 1])
        assert same_bits(one[0], ref[0][r:r + 1]) and same_bits(one[1], ref[1][off[r]:off[r + 1]]), r
    perm = np.random.default_rng(8).permutation(20)
    pr = run(m, [seqs[r] for r in perm], lists[perm])
    assert same_bits(pr[0], ref[0][perm])
    assert same_bits(pr[1], np.concatenate([ref[1][off[r]:off[r + 1]] for r in perm]))


# ---- 7: against the route that existed before: a Session replayed through the reduced histories + score_lists ----------------------------
def test_states_match_a_replayed_session(pa):
    T = geo_problem(107, n_user=12, n_item=50, n_dist=11, dim=64, len_min=1, len_max=20)
    P = spatial_init(107, T)
    m = spatial_model(pa, T, P)
    seqs = seqs_of(T)
    lists = make_lists(9, 12, T["n_item"], holes=())
    base, delta, off, keys, st = run(m, seqs, lists, return_states=True)
    red = [[int(v) for t, v in enumerate(s) if t != g] for s in seqs for g in range(len(s))]
    G = len(red)
    assert G == len(delta) == len(st["h"])
    s = m.session(G)
    s.replay(*csr(red))
    ss = s.state()
    kept = np.array([len(r) > 0 for r in red])
    assert_close(st["h"], ss["h"], "h against the session")
    assert_close(st["sts"][kept], ss["sts"][kept], "sts against the session")
    assert np.array_equal(st["last_poi"], ss["last_poi"])
    row = np.repeat(np.arange(12), np.diff(off))
    sc = s.score_lists(np.arange(G), lists[row]).cpu().numpy().astype(np.float64)
    e = assert_close(base[row] - delta, sc, "variant scores against score_lists")
    print("states against a replayed session: h %.2e, scores %.2e" % (np.abs(st["h"] - ss["h"]).max() / np.abs(ss["h"]).max(), e))


# ---- 8: bad ids on device tensors -------------------------------------------------------------------------------------------------------------
def test_bad_ids_on_device_tensors(pa):
    import torch
    T = geo_problem(108, n_user=12, n_item=50, n_dist=11, dim=64, len_min=2, len_max=20)
    P = spatial_init(108, T)
    m = spatial_model(pa, T, P)
    seqs = seqs_of(T)
    lists = make_lists(10, 12, T["n_item"])
    clean = run(m, seqs, lists)
    off, flat = csr(seqs)
    flat = flat.copy(); flat[off[2] + 1] = T["n_item"] + 3
    bad_lists = lists.copy(); bad_lists[5, 0] = T["n_item"]
    dev = lambda a: torch.as_tensor(a.astype(np.int32)).cuda()
    args = (np.zeros(12, np.int64), dev(bad_lists))
    out = explainer(m).explain(*args, histories=(dev(off), dev(flat)), sync=False)
    assert m.ctx.take_bad_ids(m._stream().value) == 2
    base, delta, goff = (o.cpu().numpy() for o in out[:3])
    assert np.array_equal(goff, clean[2])
    for r in range(12):
        rows = slice(goff[r], goff[r + 1])
        if r in (2, 5):
            assert np.isnan(base[r]).all() and np.isnan(delta[rows]).all(), r
        else:
            assert same_bits(base[r], clean[0][r]) and same_bits(delta[rows], clean[1][rows]), r
    with pytest.raises(IndexError, match="NaN"):
        explainer(m).explain(*args, histories=(dev(off), dev(flat)))
    with pytest.raises(IndexError):                                    # host arguments: before any launch
        explainer(m).explain(np.zeros(12, np.int64), bad_lists, histories=csr(seqs))
    with pytest.raises(IndexError):
        explainer(m).explain(np.zeros(12, np.int64), lists, histories=(off, flat))
    assert m.ctx.take_bad_ids(m._stream().value) == 0


# ---- 9: the rows' own train histories; evaluate.attribution_by_recency on the device ----------------------------------------------------------
def test_train_histories_and_attribution_by_recency(pa):
    T = geo_problem(109, n_user=24, n_item=50, n_dist=11, dim=64, len_min=1, len_max=20)
    P = gru_init(109, T)
    m = plain_model(pa, T, P)
    seqs = seqs_of(T)
    lists = make_lists(11, 24, T["n_item"])
    ref = run(m, seqs, lists)
    own = [o.cpu().numpy() for o in explainer(m).explain(np.arange(24), lists)]
    assert same_bits(own[0], ref[0]) and same_bits(own[1], ref[1]) and np.array_equal(own[2], ref[2]) and np.array_equal(own[3], ref[3])
    pick = np.array([5, 2, 17])
    some = [o.cpu().numpy() for o in explainer(m).explain(pick, lists[pick])]
    assert same_bits(some[0], ref[0][pick]) and same_bits(some[1], np.concatenate([ref[1][ref[2][r]:ref[2][r + 1]] for r in pick]))
    m.update_trained_users(m.predict_device(np.arange(24)))
    out = pa.evaluate.attribution_by_recency(m, [np.arange(0, 12), np.arange(12, 24)], 5)
    print("share of the attribution by position from the end:", np.round(out["share"], 3), "rows", out["rows"])
    assert out["rows"] == 24 and out["count"][0] == 24 and len(out["share"]) == max(len(s) for s in seqs)
    assert np.all(out["share"] >= 0) and float((out["share"] * out["count"]).sum()) == pytest.approx(24.0)
