"""-m gpu: the table-form recurrences of the exact forward pass with their table-row ids staged in LDS (option "xfwd_ids_lds", default 1:
te_rec_fwdxi / te_rec_fwddi / te_rec_fwd1xi, te_xfwd.hip) against the same launch with the ids loaded inside the step loop (option 0:
te_rec_fwdx<.., FT> / te_rec_fwdd<.., FT> / te_rec_fwd1x<.., FT>).  The change moves loads, no arithmetic: every comparison is BITWISE - all
nine parameter tensors (four for the plain GRU) and the (n, 5) loss rows (the plain GRU: n losses) after one training launch, the final states after a predict.
Small launches that still take the table form: a 300-POI table with 200 bins has fewer rows than a few dozen users have steps (te_setup:
2 (n_item + 1) <= steps + 192), and poi_ctx_set_exact_forward(1, 0) keeps them on the tile kernel.  Every case asserts through
poi_ctx_last_plan that the launch took the table form ("xft", and "xcomp" where the compact table is meant) and which id path it took
("xfwd_ids_lds"): a launch that silently ran the per-step-row kernel would prove nothing.

A launch of ONE sequence never takes the table form (te_setup: xft needs n > 1 - the one-sequence path forms its input rows itself), so
the "one user of length 2" case is a launch whose second tile holds exactly one user, of length 2 (one step, the shortest trainable
sequence): that workgroup stages one real entry per table and runs one step."""
import numpy as np
import pytest

from tests.gpu_util import gru_params, spatial_params, toy_problem

pytestmark = pytest.mark.gpu

SP_NAMES = ("lt", "di", "ui", "wh", "bi", "vs", "bs", "wd", "loss_weight")
GRU_NAMES = ("lt", "ui", "wh", "bi")
N_ITEM, N_DIST = 300, 200


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
    ctx.set_exact_forward(True, 1100); ctx.set_engine("auto")


def _problem(seed, n_user, dim, len_max, head=(), n_item=N_ITEM, hot=40):
    """toy_problem's padded tables with every user generated at full length and then cut to lengths drawn from 2 .. len_max, the leading
    users to the lengths in `head`."""
    T = toy_problem(seed, n_user=n_user, n_item=n_item, n_dist=N_DIST, dim=dim, len_max=len_max, min_len=len_max, hot=hot)
    lens = np.random.default_rng(seed + 1).integers(2, len_max + 1, n_user)
    lens[:len(head)] = head
    for u, L in enumerate(lens):
        T["train"][0][u, L:] = n_item; T["train"][2][u, L:] = n_item
        T["dist"][0][u, L:] = N_DIST; T["dist"][2][u, L:] = N_DIST
        T["train"][1][u, L:] = 0
    T["lens"] = lens
    return T


def _spatial(pa, T, P):
    return pa.models.OboSpatialGru(train=T["train"], test=T["test"], dist=T["dist"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                                   n_dists=[T["n_dist"], 0.2], n_in=T["dim"], n_hidden=T["dim"], init=P)


def _gru(pa, T, P):
    return pa.models.OboGru(train=T["train"], test=T["test"], alpha_lambda=[0.01, 0.001], n_user=T["n_user"], n_item=T["n_item"],
                            n_in=T["dim"], n_hidden=T["dim"], init=P)


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return a.view(np.uint32)


def _ab(pa, make, names, users, setup, want):
    """One training launch from identical tables under option 1 and option 0 -> bitwise equal tensors and loss rows; `want`: plan values
    asserted for the option-1 launch (the option-0 launch: the same with xfwd_ids_lds = 0)."""
    ctx = pa._lib.context(0)
    res = {}
    try:
        for opt in (1, 0):
            model = make()
            ctx.set_engine("tile")
            setup(ctx)
            ctx.set_option("xfwd_ids_lds", opt)
            out = np.asarray(model.train_batch(users))
            plan = {k: ctx.last_plan(k) for k in ("tile", "xft", "xcomp", "xrec1", "hyb", "xfwd_ids_lds")}
            exp = dict(want, tile=1, xft=1, xfwd_ids_lds=want.get("xfwd_ids_lds", 1) if opt else 0)
            assert {k: plan[k] for k in exp} == exp, (opt, plan, exp)
            res[opt] = (out, {k: np.asarray(getattr(model, k).get_value()) for k in names})
    finally:
        _defaults(ctx)
    assert res[1][0].shape == res[0][0].shape == ((len(users), 5) if "di" in names else (len(users),)) and np.isfinite(res[1][0]).all()
    assert np.array_equal(_bits(res[1][0]), _bits(res[0][0])), "loss rows differ between the id paths"
    for k in names:
        assert np.array_equal(_bits(res[1][1][k]), _bits(res[0][1][k])), "%s differs between the id paths" % k
    return res


def _tiles(ctx):
    ctx.set_exact_forward(True, 0)      # no per-sequence float64 kernel: 16-sequence tiles


# (dim, users, len_max, lengths of the leading users, what)
TILE_CASES = [
    (128, 48, 12, [12, 2, 12, 2, 2, 2, 12, 2, 2, 2, 2, 2, 2, 2, 2, 12], "three full tiles, the first mixes lengths 2 and len_max"),
    (128, 37, 13, [13, 2, 2, 13, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 13, 2], "partial last tile"),
    (128, 17, 26, [26] + [9] * 15 + [2], "a tile of one user of length 2"),
    (64, 48, 12, [12, 2, 12, 2, 2, 2, 12, 2, 2, 2, 2, 2, 2, 2, 2, 12], "dim 64"),
]


@pytest.mark.parametrize("dim,n,len_max,head,what", TILE_CASES, ids=[c[4] for c in TILE_CASES])
def test_tile_recurrence_ids_in_lds_is_bitwise_the_in_loop_form(pa, dim, n, len_max, head, what):
    T = _problem(8100 + dim + n, n, dim, len_max, head)
    P = spatial_params(8101 + dim, T)
    _ab(pa, lambda: _spatial(pa, T, P), SP_NAMES, np.arange(n, dtype=np.int32), _tiles, dict(xcomp=0, xrec1=0, hyb=0))


def test_plain_gru_has_no_bin_rows(pa):
    """poi_gru_step, dim 128: the side of the removed A.spatial branch without row_dp - the one bias row of ztabx for every step."""
    n, len_max = 48, 12
    T = _problem(8300, n, 128, len_max)
    P = gru_params(8301, T)
    _ab(pa, lambda: _gru(pa, T, P), GRU_NAMES, np.arange(n, dtype=np.int32), _tiles, dict(xcomp=0, xrec1=0, hyb=0))


def test_dim_256_table_form(pa):
    """te_rec_fwdd<256, FT>: at dim 256 the table form is the compact table's alone (te_setup) - switched on for a 20-user launch."""
    n, len_max = 20, 12
    T = _problem(8400, n, 256, len_max)
    P = spatial_params(8401, T)

    def setup(ctx):
        ctx.set_regroup_min(0); ctx.set_option("forward_table_compact_min", 0)
    _ab(pa, lambda: _spatial(pa, T, P), SP_NAMES, np.arange(n, dtype=np.int32), setup, dict(xcomp=1, xrec1=0, hyb=0))


def test_per_sequence_table_form(pa):
    """te_rec_fwd1x<.., FT>: the default per_sequence_max, 40 users."""
    n, len_max = 40, 12
    T = _problem(8500, n, 128, len_max)
    P = spatial_params(8501, T)
    _ab(pa, lambda: _spatial(pa, T, P), SP_NAMES, np.arange(n, dtype=np.int32), lambda ctx: None, dict(xcomp=0, xrec1=1, hyb=0))


def test_id_table_that_does_not_fit_takes_the_in_loop_loads(pa):
    """dim 128: 121,344 bytes of digit planes and fragments + 256 bytes of ids per step against the 152 KB opt-in - a table of 134 entries (133 steps and
    the one the loop requests past the end) fits, the 140 entries of 140-position sequences do not: option 1 reports xfwd_ids_lds = 0 and computes what option 0 computes."""
    n, len_max = 20, 140
    T = _problem(8600, n, 128, len_max, [140, 2, 140, 2] + [30] * 16)
    P = spatial_params(8601, T)
    _ab(pa, lambda: _spatial(pa, T, P), SP_NAMES, np.arange(n, dtype=np.int32), _tiles, dict(xcomp=0, xrec1=0, hyb=0, xfwd_ids_lds=0))


def test_compact_table(pa):
    """1536 users of length <= 6, the smallest launch forward_table_compact_min admits, dim 128: the ids are the ranks te_gather wrote
    (row_pc); at this size the hybrid recurrences run the tiles next to the per-sequence kernel."""
    n, len_max = 1536, 6
    T = _problem(8700, n, 128, len_max, n_item=2500, hot=400)
    P = spatial_params(8701, T)
    _ab(pa, lambda: _spatial(pa, T, P), SP_NAMES, np.arange(n, dtype=np.int32), lambda ctx: None, dict(xcomp=1, xrec1=0))


def test_predict_final_states_in_the_callers_order(pa):
    """te_rec_fwdx<.., true, PRED>: hts bitwise between the id paths, and row k of the result is user ids[k] whatever order the launch ran in."""
    n, len_max = 48, 12
    T = _problem(8800, n, 128, len_max)
    P = spatial_params(8801, T)
    ctx = pa._lib.context(0)
    ids = np.random.default_rng(8).permutation(n).astype(np.int32)
    res = {}
    try:
        for opt in (1, 0):
            model = _spatial(pa, T, P)
            ctx.set_engine("tile"); _tiles(ctx); ctx.set_option("xfwd_ids_lds", opt)
            model.train_batch(np.arange(n, dtype=np.int32))      # (the same shape takes the table form as a training launch: the plan says so)
            assert ctx.last_plan("xft") == 1 and ctx.last_plan("xrec1") == 0 and ctx.last_plan("xfwd_ids_lds") == opt
            model.update_trained_items(); model.update_trained_dists()
            hts, sts = model.predict(ids)
            assert ctx.last_plan("xfwd_ids_lds") == opt      # (the value the predict launch recorded)
            hts_id, _ = model.predict(np.arange(n, dtype=np.int32))
            res[opt] = (np.asarray(hts), np.asarray(sts), np.asarray(hts_id))
    finally:
        _defaults(ctx)
    assert res[1][0].shape == (n, 128) and np.isfinite(res[1][0]).all() and np.abs(res[1][0]).max() > 0
    assert np.array_equal(_bits(res[1][0]), _bits(res[0][0])), "hts differ between the id paths"
    assert np.array_equal(_bits(res[1][1]), _bits(res[0][1])), "sts differ between the id paths"
    assert np.array_equal(_bits(res[1][0]), _bits(res[1][2][ids])), "hts rows are not in the caller's order"
