"""-m gpu: the exact forward pass (csrc/te_xfwd.hip: te_xpack, te_xztab, te_gemmx<64|128|256>, te_rec_fwdx, te_rec_fwd1x, te_rec_fwdd) on
weights OUTSIDE the reference's uniform(-0.5, 0.5) init, which every other module draws from - the regimes of tests/xfwd_cases.py: row
maxima at exact powers of two and one float32 below (the |Q| <= 2^38 boundary), rows 2^-20 .. 2^1 apart, entries spread over every
digit plane, extreme digits with equal signs on both operands (the int32 class sums and merges as large as float32 rows make them),
zero and subnormal rows, tiny and huge tables (h = +-1 exactly), a trained model's spread of row norms.

The judge is the float64 oracle (O.spatial_predict / O.gru_predict / O.spatial_step); tests/test_xfwd_cases_cpu.py shows on the CPU
that every launch here is well conditioned (float64 vs longdouble <= 1e-11) and that the documented scheme is able to pass.  The bars:
predict - hts and sts within 2e-6 (what tests/test_gpu_tile_engine.py holds the exact forward pass to); training step - the suite's
standing assert_step_close bars on the tile engine, and tests/test_gpu_exact.py's 2e-7 / 1e-6 on the exact engine for the same
launches (which tells a forward defect from float32 backward noise).

Kernel forms are forced with the existing switches and, for training launches, asserted through poi_ctx_last_plan."""
import functools

import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import xfwd_cases as C
from tests.gpu_util import assert_close, assert_step_close, batch_mean_update, rel_err

pytestmark = pytest.mark.gpu

SP_NAMES = ("lt", "di", "ui", "wh", "bi", "vs", "bs", "wd", "loss_weight")
BAR = 2e-6                       # predict: hts / sts against the float64 oracle
XTOL, XDELTA = 2e-7, 1e-6        # exact engine (tests/test_gpu_exact.py)
WORST = {}                       # (regime, dim) -> worst hts / sts error seen (printed by the module's last test)

# (name, per_sequence_max, xfwd_ids_lds): int8 tiles with the table-row ids in LDS / loaded in the loop; the per-sequence float64 kernel
# (dim 256 has none: te_rec_fwdd either way)
FORMS = (("int8-tiles", 0, 1), ("int8-tiles-ids-in-loop", 0, 0), ("per-sequence-f64", 512, 1))


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available()
    import poi_amd
    poi_amd._lib.load()
    yield poi_amd
    _defaults(poi_amd._lib.context(0))


def _defaults(ctx):
    ctx.set_option("xfwd_ids_lds", 1); ctx.set_option("forward_table_compact_min", 1536); ctx.set_regroup_min(1280)
    ctx.set_exact_forward(True, 1100); ctx.set_one_sequence_path(True); ctx.set_engine("auto")


def _model(pa, c, T, P):
    if c.spatial:
        return pa.models.OboSpatialGru(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"],
                                       n_item=T["n_item"], n_dists=[T["n_dist"], 0.2], n_in=c.dim, n_hidden=c.dim, init=P)
    return pa.models.OboGru(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                            n_in=c.dim, n_hidden=c.dim, init=P)


@functools.lru_cache(maxsize=None)
def _oracle_predict(c):
    """(T, P, hts, sts) of the float64 oracle, computed once per case and shared."""
    T = C.problem(c); P = C.params(c)
    if c.spatial:
        eh, es = O.spatial_predict(P, P["lt"], P["di"], T["train"][0], T["dist"][0], T["train"][1])
    else:
        eh, es = O.gru_predict(P, P["lt"], T["train"][0], T["train"][1]), None
    for a in (eh, es):
        if a is not None:
            a.setflags(write=False)
    return T, P, eh, es


_DEVICE = {}


def _device_predict(pa, c):
    """{form: (hts, sts)} of the case on the device, one predict launch per kernel form, computed once per case and shared."""
    if c in _DEVICE:
        return _DEVICE[c]
    T, P, eh, es = _oracle_predict(c)
    ctx = pa._lib.context(0)
    res = {}
    try:
        for name, per_seq, ids_lds in FORMS:
            model = _model(pa, c, T, P)
            ctx.set_engine("tile"); ctx.set_exact_forward(True, per_seq); ctx.set_option("xfwd_ids_lds", ids_lds)
            model.update_trained_items()
            if c.spatial:
                model.update_trained_dists()
            out = model.predict(np.arange(c.n_seq, dtype=np.int32))
            res[name] = (np.asarray(out[0]), np.asarray(out[1])) if c.spatial else (np.asarray(out), None)
    finally:
        _defaults(ctx)
    _DEVICE[c] = res
    return res


@pytest.mark.parametrize("c", C.PREDICT_CASES, ids=C.case_id)
def test_predict_final_states_meet_the_oracle_in_every_regime(pa, c):
    """hts of every kernel form within 2e-6 of the float64 oracle.  n_item 60: the forward table over the whole POI table (te_gemmx
    over table rows, zero pad row included); n_item 3000: one gathered row per step.
    Measured: 2.97e-08 .. 5.0e-08 in every regime, dim and form - the float32 rounding of the stored state."""
    T, P, eh, es = _oracle_predict(c)
    w = WORST.setdefault((c.regime, c.dim), [0.0, 0.0])
    errs = {}
    for name, (hts, _) in _device_predict(pa, c).items():
        assert hts.shape == eh.shape
        errs[name] = rel_err(hts, eh) if np.isfinite(hts).all() else float("inf")
        print("%s %s: hts %.2e" % (C.case_id(c), name, errs[name]))
        w[0] = max(w[0], errs[name])
    for name, e in errs.items():
        assert e <= BAR, "hts of %s (%s): %.3e > %.1e" % (C.case_id(c), name, e, BAR)


@pytest.mark.parametrize("c", [c for c in C.PREDICT_CASES if c.spatial], ids=C.case_id)
def test_predict_bin_probabilities_meet_the_oracle_in_every_regime(pa, c):
    """sts = softmax(vs . h + bs) of the same launches within 2e-6 of the float64 oracle.  Under the exact forward pass predict forms
    them in float64 from the stored final states (te_xsts, csrc/te_xfwd.hip): measured 2.7e-08 .. 8.6e-08 in every regime, dim and form.
    This test found why: predict's float32 head (te_head: float32-input MFMAs over K = dim) left 1.3e-07 .. 5.5e-07 at dim 64,
    4.2e-07 .. 1.8e-06 at dim 128, 9.1e-07 .. 1.9e-06 at dim 256 and 3.20e-06 - over the bar - on trained4 at dim 256 (|h| ~ 1,
    |logit| up to 14), with final states 2.98e-08 from the oracle in the same launch."""
    T, P, eh, es = _oracle_predict(c)
    w = WORST.setdefault((c.regime, c.dim), [0.0, 0.0])
    errs = {}
    for name, (_, sts) in _device_predict(pa, c).items():
        assert sts.shape == es.shape
        errs[name] = rel_err(sts, es) if np.isfinite(sts).all() else float("inf")
        print("%s %s: sts %.2e" % (C.case_id(c), name, errs[name]))
        w[1] = max(w[1], errs[name])
    for name, e in errs.items():
        assert e <= BAR, "sts of %s (%s): %.3e > %.1e" % (C.case_id(c), name, e, BAR)


@pytest.mark.parametrize("c", [c for c in C.PREDICT_CASES if c.regime == "huge"], ids=C.case_id)
def test_saturated_states_are_exactly_one(pa, c):
    """huge: wherever the oracle's float64 final state is +-1 exactly, the device's is +-1.0f - the chain carried Q = +-2^38 (leading
    digit +-64) through x_digits38 and the clamped gates without a wrong digit, in every kernel form."""
    T, P, eh, es = _oracle_predict(c)
    one = np.abs(eh) == 1.0
    assert one.sum() >= 100, "the regime does not saturate"
    for name, (hts, _) in _device_predict(pa, c).items():
        assert np.isfinite(hts).all() and np.abs(hts).max() <= 1.0, name
        assert np.array_equal(hts[one], eh[one].astype(np.float32)), "%s: %d of %d saturated states are not +-1.0f" % (name, int((hts[one] != eh[one]).sum()), int(one.sum()))


# ------------------------------------------------------------------------------------------------
# one training step
# ------------------------------------------------------------------------------------------------
def _get(model):
    out = {}
    for k in SP_NAMES:
        v = getattr(model, k).get_value()
        out[k] = float(v) if k == "wd" else v
    return out


@functools.lru_cache(maxsize=None)
def _oracle_step(c):
    T = C.problem(c); P = C.params(c)
    Pm, Qm, DPm, DQm, Mm = T["train"][0], T["train"][2], T["dist"][0], T["dist"][2], T["train"][1]
    news, touched, outs = [], [], []
    for u in range(c.n_seq):
        Pn, out = O.spatial_step(P, Pm[u], Qm[u], DPm[u], DQm[u], Mm[u], 0.01, 0.001)
        news.append(Pn); outs.append(out)
        touched.append(dict(lt=np.unique(np.concatenate((Pm[u], Qm[u]))), di=np.unique(DPm[u])))
    exp = news[0] if c.n_seq == 1 else batch_mean_update(P, news, touched, ("lt", "di"), ("ui", "wh", "bi", "vs", "bs", "wd", "loss_weight"))
    return T, P, exp, outs


def _plan_wanted(c, form):
    """The form te_setup gives these launches (asserted, so that a launch that quietly took another kernel proves nothing).
    "tiles": exact_forward(1, 0), regroup_min(0), forward_table_compact_min 0 - int8 tiles (dim 256: te_rec_fwdd) over a forward table,
    the compact one where the per-POI regrouping runs (dims >= 128); "per-sequence": the defaults - te_rec_fwd1x at dims <= 128, the
    whole-table form where the table is small against the launch (60 POIs), per-step rows otherwise."""
    if c.n_seq == 1:
        return dict(tile=1, one=1 if c.dim <= 128 else 0, xft=0, xrec1=1 if (form == "per-sequence" and c.dim <= 128) else 0)
    if form == "tiles":
        return dict(tile=1, one=0, xrec1=0, xft=1, xcomp=1 if c.dim >= 128 else 0)
    return dict(tile=1, one=0, xrec1=1 if c.dim <= 128 else 0, xft=1 if (c.n_item == 60 and c.dim <= 128) else 0, xcomp=0)


@pytest.mark.parametrize("c", C.STEP_CASES, ids=C.case_id)
def test_one_training_step_meets_the_oracle(pa, c):
    """One launch over all the case's sequences (one sequence: the reference step; more: the mean rule) on the tile engine in both forms
    of the exact forward pass at the suite's standing bars, and on the exact engine at 2e-7 / 1e-6."""
    T, P, exp, outs = _oracle_step(c)
    ctx = pa._lib.context(0)
    users = np.arange(c.n_seq, dtype=np.int32)
    try:
        for form in ("tiles", "per-sequence", "exact-engine"):
            model = _model(pa, c, T, P)
            _defaults(ctx)
            if form == "exact-engine":
                ctx.set_engine("exact")
            else:
                ctx.set_engine("tile")
                if form == "tiles":
                    ctx.set_exact_forward(True, 0); ctx.set_regroup_min(0); ctx.set_option("forward_table_compact_min", 0)
            got_out = np.asarray(model.train_batch(users))
            if form != "exact-engine":
                want = _plan_wanted(c, form)
                plan = {k: ctx.last_plan(k) for k in want}
                assert plan == want, (form, plan, want)
            for k, out in enumerate(outs):
                assert_close(got_out[k][:3], out[:3], "%s losses[%d]" % (form, k), rtol=1e-6 if form == "exact-engine" else 2e-5)
            got = _get(model)
            if form == "exact-engine":
                worst = assert_step_close(got, exp, P, SP_NAMES, form, rtol=XTOL, delta_rtol=XDELTA)
            else:
                worst = assert_step_close(got, exp, P, SP_NAMES, form)
            print("%s %s: worst tensor %.2e" % (C.case_id(c), form, worst))
    finally:
        _defaults(ctx)


def test_report_worst_errors_per_regime(pa):
    """(runs last in the module: the table of DESIGN.md section 2 - with -s)"""
    for (regime, dim), (eh, es) in sorted(WORST.items()):
        print("worst predict error  %-15s dim %3d: hts %.2e  sts %.2e" % (regime, dim, eh, es))
    assert all(np.isfinite(v).all() for v in WORST.values())
    _DEVICE.clear()
