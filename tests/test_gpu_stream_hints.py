"""-m gpu: the streaming-store hint of the exact forward recurrence (option "stream_hints", default 1; te_xfwd.hip te_rec_fwdx_kernel_nt /
te_rec_fwdxi_kernel_nt: the 16-sequence tiles store G, H and RH non-temporally) against the same launch with plain stores (option 0).  A
cache hint moves no value and reorders no sum: every comparison is BITWISE - all nine parameter tensors and the (n, 5) loss rows after one
training launch from the same initial model - and the hinted launch also meets the oracle bars of tests/test_gpu_tile_engine.py.

The product applies the hint to launches of at least "stream_hints_min" (2560) sequences only; the cases here set it to 0 so that the
smallest launch that reaches a kernel runs its hinted instance, and assert through poi_ctx_last_plan ("stream_hints") that it did: a launch
that silently ran the plain kernel would prove nothing.  The per-sequence kernels (te_rec_fwd1x / te_rec_bwd1), te_head3, the backward
recurrence, te_psum / te_dsum / te_wgrad and dim 256 have no hinted instance (measured and taken out: docs/NOTEBOOK.md, stream hints) -
their cases check that the option is harmless there and that the plan says 0."""
import numpy as np
import pytest

from tests.gpu_util import assert_close, assert_step_close, spatial_params, toy_problem
from tests.test_gpu_tile_engine import SP_NAMES, _get, _model, _oracle_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    poi_amd._lib.load()
    yield poi_amd
    _defaults(poi_amd._lib.context(0))


def _defaults(ctx):
    ctx.set_option("stream_hints", 1); ctx.set_option("stream_hints_min", 2560)
    ctx.set_regroup_min(1280); ctx.set_exact_forward(True, 1100); ctx.set_small_launch(1800); ctx.set_engine("auto")


def _tiles(ctx):
    ctx.set_engine("tile"); ctx.set_exact_forward(True, 0); ctx.set_small_launch(0)      # 16-sequence tiles, forward and backward


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _on_off(pa, make, users, setup, want):
    """One training launch from the same initial model with the hints on and off -> {opt: (loss rows, tensors)}, asserted bitwise equal.
    `want`: plan values of both launches; "stream_hints" in it is the value expected of the option-1 launch (option 0: always 0)."""
    ctx = pa._lib.context(0)
    res = {}
    try:
        for opt in (1, 0):
            model = make()
            setup(ctx)
            ctx.set_option("stream_hints_min", 0); ctx.set_option("stream_hints", opt)
            out = np.asarray(model.train_batch(users))
            exp = dict(want, stream_hints=want["stream_hints"] if opt else 0)
            plan = {k: ctx.last_plan(k) for k in exp}
            assert plan == exp, (opt, plan, exp)
            res[opt] = (out, _get(model), model)
    finally:
        _defaults(ctx)
    assert res[1][0].shape == res[0][0].shape == (len(users), 5) and np.isfinite(res[1][0]).all()
    assert np.array_equal(_bits(res[1][0]), _bits(res[0][0])), "loss rows differ between hinted and plain stores"
    for k in SP_NAMES:
        assert np.array_equal(_bits(res[1][1][k]), _bits(res[0][1][k])), "%s differs between hinted and plain stores" % k
    return res


def _meets_the_oracle(P, T, users, out, got, what):
    exp, outs = _oracle_batch(P, T, users)
    for k, o in enumerate(outs):
        assert_close(out[k][:3], o[:3], "%s losses[%d]" % (what, k), rtol=2e-5)
    assert_step_close(got, exp, P, SP_NAMES, what)


@pytest.mark.parametrize("dim", [64, 128])
def test_per_step_row_forward(pa, dim):
    """te_rec_fwdx<D, false>: 150 users of length <= 14 (ten tiles, the last one partial) over a POI table too large for the forward table."""
    n = 150
    T = toy_problem(9100 + dim, n_user=n, n_item=1500, n_dist=60, dim=dim, len_max=14, hot=60)
    P = spatial_params(9101 + dim, T)
    users = np.random.default_rng(5).permutation(n).astype(np.int32)
    res = _on_off(pa, lambda: _model(pa, T, P), users, _tiles, dict(tile=1, xft=0, xrec1=0, rec1=0, hyb=0, stream_hints=1))
    _meets_the_oracle(P, T, users, res[1][0], res[1][1], "dim %d, hinted stores" % dim)


def test_compact_table_with_ids_in_lds_inside_the_hybrid_window(pa):
    """te_rec_fwdxi<128>: 1600 length-sorted users of length <= 12 under the product's own plan - the compact forward table (from 1536
    sequences), its ids in LDS, and the hybrid recurrences (1150 .. 2300 sequences): the leading sequences run on te_rec_fwd1x (plain
    stores) WHILE the tiles store with the hint."""
    from oracle import c_oracle as C
    from poi_amd.data import padded_to_csr
    n = 1600
    T = toy_problem(9300, n_user=n, n_item=2500, n_dist=200, dim=128, len_max=12, min_len=2, hot=400)
    P = spatial_params(9301, T)
    lens = np.asarray(T["lens"])
    users = np.argsort(-lens, kind="stable").astype(np.int32)
    res = _on_off(pa, lambda: _model(pa, T, P), users, lambda ctx: None, dict(tile=1, xft=1, xcomp=1, xfwd_ids_lds=1, xrec1=0, hyb=1, stream_hints=1))
    ctx = pa._lib.context(0)
    res[1][2].train_batch(users)      # (the split is read back from the device: the plan of one more launch of the same users)
    lead = ctx.last_plan("hyb_fwd_seq")
    assert 0 < lead < n, "the hybrid split is trivial (%d of %d sequences per sequence): the tiles and the per-sequence kernel did not run side by side" % (lead, n)
    off, p = padded_to_csr(T["train"][0], lens); _, q = padded_to_csr(T["train"][2], lens)
    _, dp = padded_to_csr(T["dist"][0], lens); _, dq = padded_to_csr(T["dist"][2], lens)
    exp, eout, _ = C.spatial_batch_mean(P, off, p, q, dp, dq, users, T["len_max"], 0.01, 0.001, threads=8)
    assert_close(res[1][0][:, :3], eout[:, :3], "losses vs oracle", rtol=2e-5)
    assert_step_close(res[1][1], exp, P, SP_NAMES, "1600 users, hinted stores")


def test_per_sequence_kernels_have_no_hinted_instance(pa):
    """64 users, dim 128, the product's own plan: te_rec_fwd1x / te_rec_bwd1.  The option changes nothing there and the plan says so."""
    n = 64
    T = toy_problem(9400, n_user=n, n_item=400, n_dist=60, dim=128, len_max=14, hot=60)
    P = spatial_params(9401, T)
    users = np.arange(n, dtype=np.int32)
    res = _on_off(pa, lambda: _model(pa, T, P), users, lambda ctx: ctx.set_engine("tile"), dict(tile=1, xrec1=1, rec1=1, hyb=0, stream_hints=0))
    _meets_the_oracle(P, T, users, res[1][0], res[1][1], "per-sequence kernels")


def test_half_poi_table(pa):
    """table_dtype="f16", dim 128, 150 users in tiles: the hinted launch is bitwise the plain one (lt compared as stored, in half) and meets
    the bars of test_fp16_poi_table_float32_math - float32 tensors against the oracle run from the half-rounded table, lt within one half ulp."""
    n, dim = 150, 128
    T = toy_problem(9500, n_user=n, n_item=1500, n_dist=40, dim=dim, len_max=14, hot=100)
    P = spatial_params(9501, T)
    P["lt"] = np.asarray(P["lt"], np.float16).astype(np.float64)
    users = np.random.default_rng(6).permutation(n).astype(np.int32)

    def make():
        return pa.models.OboSpatialGru(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=n, n_item=T["n_item"],
                                       n_dists=[T["n_dist"], 0.2], n_in=dim, n_hidden=dim, init=P, table_dtype="f16")
    res = _on_off(pa, make, users, _tiles, dict(tile=1, xft=0, xrec1=0, rec1=0, stream_hints=1))
    import torch
    assert res[1][2].lt.t.dtype == torch.float16 and torch.equal(res[1][2].lt.t, res[0][2].lt.t)
    exp, outs = _oracle_batch(P, T, users)
    out, got = res[1][0], res[1][1]
    for k, o in enumerate(outs):
        assert_close(out[k][:3], o[:3], "losses[%d]" % k, rtol=2e-5)
    assert_step_close(got, exp, P, [k for k in SP_NAMES if k != "lt"], "fp16 table, hinted stores")
    lt = np.asarray(got["lt"], np.float64)
    want = np.asarray(exp["lt"], np.float16).astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    assert (np.abs(lt - want) <= ulp + 1e-5 * np.abs(want).max()).all(), "lt differs from half(oracle) by more than one half ulp"
    assert (lt == want).mean() > 0.98, "more than 2 % of the half elements rounded the other way"


def test_predict_is_untouched(pa):
    """predict_device, dim 128, 150 users in tiles: a predict launch stores no per-step rows and has no hinted instance - hts and sts are
    bitwise equal under both option values."""
    n = 150
    T = toy_problem(9600, n_user=n, n_item=1500, n_dist=60, dim=128, len_max=14, hot=60)
    P = spatial_params(9601, T)
    ids = np.random.default_rng(7).permutation(n).astype(np.int32)
    ctx = pa._lib.context(0)
    res = {}
    try:
        for opt in (1, 0):
            model = _model(pa, T, P)
            _tiles(ctx); ctx.set_option("stream_hints_min", 0); ctx.set_option("stream_hints", opt)
            model.update_trained_items(); model.update_trained_dists()
            h, s = model.predict_device(ids)
            res[opt] = (h.cpu().numpy(), s.cpu().numpy())
    finally:
        _defaults(ctx)
    assert res[1][0].shape == (n, 128) and np.isfinite(res[1][0]).all() and np.abs(res[1][0]).max() > 0
    assert np.array_equal(_bits(res[1][0]), _bits(res[0][0])), "hts differ"
    assert np.array_equal(_bits(res[1][1]), _bits(res[0][1])), "sts differ"
