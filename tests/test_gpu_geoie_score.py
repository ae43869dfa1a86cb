"""GeoIE's trained score rule on the device (csrc/geoie_score.hip, poi_geoie_score_all_geo / poi_geoie_score_topk_geo, models.OboGeoIE
rule="geo", score_new / recommend_new / rank_new) against the float64 oracle of tests/geoie_score_oracle.py.

Tolerance of the matrix: every finite score within 1e-5 M(l) of the oracle, M the absolute mass the oracle returns.  A float32 dot product
of D <= 128 terms errs by at most D 2^-24 = 7.6e-6 of its absolute mass, one float32 ulp of d moves f by |b| 1.2e-7, everything else is
float64.  The top-K is checked against the DEVICE matrix, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from poi_amd import _lib, data as D, evaluate as E, harness
from poi_amd.models import OboGeoIE
from tests import geoie_oracle as O
from tests import geoie_score_oracle as S
from tests import rank_oracle as R

pytestmark = pytest.mark.gpu

P_ = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
N_ITEM = 2085            # 8 spans of 256 and a ragged tail of 37; 2 of 1024 and 37; not a multiple of 16
N_HIST = 70
TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.context(0)
    yield c
    c.set_option("geoie_score_span", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(v):
    return torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).cuda()


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists]) if off[-1] else np.zeros(0, np.int64)
    return off, flat


class Problem:
    """Tables, places and 70 histories: 0 / 1 / 2 / 17 / 64 / 65 / 130 distinct POIs, 50 check-ins over 6 POIs, 62 random ones with
    revisits.  153 POIs are exact copies of another POI (g / h / z rows and place): exact score ties, some of them across spans.  POI 41
    shares its place - and nothing else - with POI 40."""

    def __init__(self, dim, b, seed=1):
        rng = np.random.default_rng(seed * 1000 + dim)
        P = O.round_f32(O.init_tables(rng, N_HIST, N_ITEM, dim))
        P["a"], P["b"] = 0.37, float(b)
        coords = np.stack([40 + 0.3 * rng.random(N_ITEM), -74 + 0.4 * rng.random(N_ITEM)], 1)
        pairs = [(int(d), int(s)) for d, s in zip(rng.permutation(np.arange(50, N_ITEM))[:150], rng.integers(50, N_ITEM, 150))] + [(11, 10), (1500, 10)]
        for d, s in pairs:
            for k in ("g", "h", "z"):
                P[k][d] = P[k][s]
            coords[d] = coords[s]
        coords[41] = coords[40]
        hist = [rng.permutation(N_ITEM)[:n] for n in (0, 1, 2, 17, 64, 65, 130)]
        rest = rng.permutation(N_ITEM)
        hist[3] = np.concatenate(([40, 10], rest[~np.isin(rest, (40, 10))][:15]))          # the planted places are in a history
        hist.append(rng.choice(rng.permutation(N_ITEM)[:6], 50))
        while len(hist) < N_HIST:
            h = rng.integers(0, N_ITEM, rng.integers(1, 61))
            for i in np.nonzero(rng.random(len(h)) < 0.3)[0]:
                if i > 0:
                    h[i] = h[rng.integers(0, i)]
            hist.append(h)
        self.P, self.coords, self.hist, self.dim = P, coords, [np.asarray(h, np.int64) for h in hist], dim
        self.T = {k: torch.as_tensor(P[k], dtype=torch.float32).cuda().contiguous() for k in O.TABLES}
        self.ab = torch.tensor([P["a"], P["b"]], dtype=torch.float64, device="cuda")
        self.xy = torch.as_tensor(np.ascontiguousarray(coords)).cuda()
        self.cphi = torch.as_tensor(D.cos_lat(coords)).cuda()
        comp = [S.compact(h) for h in self.hist]
        off, flat = _csr([c[0] for c in comp])
        self.off, self.p, self.mult = _i32(off), _i32(np.append(flat, 0)), _i32(np.append(_csr([c[1] for c in comp])[1], 1))
        self._oracle = {}

    def prm(self):
        return _lib.GeoieParams(*[P_(self.T[k]) for k in O.TABLES], P_(self.ab), N_HIST, N_ITEM, self.dim)

    def oracle(self, r, with_tu, d_min):
        key = (int(r), bool(with_tu), d_min)
        if key not in self._oracle:
            self._oracle[key] = S.scores_geo(self.P, self.hist[r], self.coords, d_min, self.P["t"][r] if with_tu else None)
        return self._oracle[key]

    def _args(self, rows, with_tu):
        sel = np.arange(N_HIST) if rows is None else np.asarray(rows, np.int64)
        tu = self.T["t"][torch.as_tensor(sel).cuda()].contiguous() if with_tu else None
        return sel, (None if rows is None else _i32(sel)), tu

    def matrix(self, ctx, rows=None, with_tu=True, d_min=0.01, csr=None):
        sel, rr, tu = self._args(rows, with_tu)
        off, p, mult = csr or (self.off, self.p, self.mult)
        out = torch.full((len(sel), N_ITEM), 7.0, dtype=torch.float32, device="cuda")
        prm = self.prm()
        ctx.check(ctx.lib.poi_geoie_score_all_geo(ctx.handle, ctypes.byref(prm), P_(off), P_(p), P_(mult), P_(tu), P_(rr), len(sel), P_(self.xy),
                                                  P_(self.cphi), d_min, P_(out), _stream()))
        return out.cpu().numpy()

    def topk(self, ctx, k, rows=None, with_tu=True, d_min=0.01, ex=None, csr=None):
        sel, rr, tu = self._args(rows, with_tu)
        off, p, mult = csr or (self.off, self.p, self.mult)
        idx = torch.full((len(sel), k), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((len(sel), k), 7.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((len(sel),), -7, dtype=torch.int32, device="cuda")
        eo, el = (_i32(ex[0]), _i32(np.append(ex[1], 0))) if ex is not None else (None, None)
        prm = self.prm()
        ctx.check(ctx.lib.poi_geoie_score_topk_geo(ctx.handle, ctypes.byref(prm), P_(off), P_(p), P_(mult), P_(tu), P_(rr), len(sel), P_(self.xy),
                                                   P_(self.cphi), d_min, P_(eo), P_(el), k, P_(idx), P_(sc), P_(cnt), _stream()))
        return idx.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()


_PROBLEMS = {}


def problem(dim, b):
    if (dim, b) not in _PROBLEMS:
        _PROBLEMS[(dim, b)] = Problem(dim, b)
    return _PROBLEMS[(dim, b)]


def _check_rows(X, got, sel, with_tu, d_min, what):
    """Each finite score within TOL M of the oracle, NaN where the oracle is NaN; returns (candidates, candidates with M > 1e3 |S|)."""
    n_all = n_thin = 0
    for i, r in enumerate(sel):
        want, M = X.oracle(r, with_tu, d_min)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[i]), nan), (what, r)
        err = np.abs(got[i][~nan].astype(np.float64) - want[~nan])
        worst = int(np.argmax(err - TOL * M[~nan])) if err.size else 0
        assert np.all(err <= TOL * M[~nan]), (what, r, err[worst], M[~nan][worst])
        n_all += int((~nan).sum())
        n_thin += int((M[~nan] > 1e3 * np.abs(want[~nan])).sum())
    return n_all, n_thin


def _expected_topk(row, excluded, k):
    """Stable descending sort of a device score row over the selectable candidates: (ids, scores, count)."""
    cand = np.ones(len(row), bool)
    cand[np.asarray(excluded, np.int64)] = False
    with np.errstate(invalid="ignore"):
        cand &= row > -np.inf                                                              # NaN and -inf are never selected
    ids = np.nonzero(cand)[0]
    top = ids[np.lexsort((ids, -row[ids]))][:k]
    idx, sc = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32)
    idx[:len(top)], sc[:len(top)] = top, row[top]
    return idx, sc, int(cand.sum())


@pytest.mark.parametrize("b", [-0.8, 0.7])
@pytest.mark.parametrize("dim", [4, 20, 64, 128])
def test_matrix_parity(ctx, dim, b):
    X = problem(dim, b)
    ctx.set_option("geoie_score_span", 0)
    ctx.take_bad_ids()
    full = X.matrix(ctx)                                                                    # 70 rows, rows = NULL, tu given
    n_all, n_thin = _check_rows(X, full, range(N_HIST), True, 0.01, "70 rows")
    # the bar is not vacuous: the absolute mass is within 1e3 of the score on at least 95 % of the candidates
    assert n_thin <= 0.05 * n_all, (n_thin, n_all)
    five = [6, 3, 7, 0, 5]                                                                  # shuffled rows, tu = NULL (the unseen user)
    got = X.matrix(ctx, rows=five, with_tu=False)
    n_all, n_thin = _check_rows(X, got, five, False, 0.01, "5 rows")
    assert n_thin <= 0.05 * n_all, (n_thin, n_all)
    assert np.all(got[3] == 0.0)                                                            # an empty history without a user term
    # a row's bits do not depend on the other rows of the call: 1 / 3 rows and a shuffled 70-row call against the first call
    assert np.array_equal(X.matrix(ctx, rows=[4]), full[[4]])
    assert np.array_equal(X.matrix(ctx, rows=[6, 1, 2]), full[[6, 1, 2]])
    perm = np.random.default_rng(dim).permutation(N_HIST)
    assert np.array_equal(X.matrix(ctx, rows=perm), full[perm])
    for span in (256, 1024, 4096):                                                          # 9, 3 and 1 spans per row
        ctx.set_option("geoie_score_span", span)
        assert np.array_equal(X.matrix(ctx, rows=five), full[five]), span
        assert ctx.last_plan("geoie_score_splits") == -(-N_ITEM // span) and ctx.last_plan("geoie_score_span") == span
    ctx.set_option("geoie_score_span", 0)
    assert ctx.take_bad_ids() == 0


def _same_place(X, hist):
    """Candidates at the place of a history POI."""
    xy = X.coords
    here = {tuple(xy[k]) for k in hist}
    return np.array([tuple(xy[l]) in here for l in range(N_ITEM)])


def test_zero_distance_without_d_min(ctx):
    rows = [3, 7, 20, 0]
    # b < 0: exactly the candidates at a history POI's place are NaN - the history's own POIs, the place twin 41 of 40, the copies of 10
    X = problem(20, -0.8)
    got = X.matrix(ctx, rows=rows, d_min=0.0)
    _check_rows(X, got, rows, True, 0.0, "b < 0, d_min = 0")
    for i, r in enumerate(rows):
        assert np.array_equal(np.isnan(got[i]), _same_place(X, X.hist[r])), r
    assert all(np.isnan(got[0][l]) for l in (40, 41, 10, 11, 1500)) and not np.isnan(got[3]).any()
    idx, sc, cnt = X.topk(ctx, 32, rows=rows, d_min=0.0)
    for i, r in enumerate(rows):
        nan = np.isnan(got[i])
        assert not nan[idx[i]].any() and cnt[i] == N_ITEM - nan.sum()
        e_idx, e_sc, _ = _expected_topk(got[i], [], 32)
        assert np.array_equal(idx[i], e_idx) and np.array_equal(sc[i], e_sc)
    # b > 0: those pairs contribute 0 and every score is finite
    Y = problem(20, 0.7)
    got = Y.matrix(ctx, rows=rows, d_min=0.0)
    assert np.isfinite(got).all()
    _check_rows(Y, got, rows, True, 0.0, "b > 0, d_min = 0")


def _exclusions(X, rng):
    """Row r: no list (r % 3 == 0), its whole history (1), everything but 5 POIs (2: a short row)."""
    lists = []
    for r in range(N_HIST):
        if r % 3 == 0:
            lists.append(np.zeros(0, np.int64))
        elif r % 3 == 1:
            lists.append(np.unique(X.hist[r]))
        else:
            lists.append(np.setdiff1d(np.arange(N_ITEM), rng.permutation(N_ITEM)[:5]))
    return lists


@pytest.mark.parametrize("k", [1, 20, 32])
def test_topk_equals_the_sorted_device_matrix(ctx, k):
    X = problem(64, -0.8)
    ctx.set_option("geoie_score_span", 0)
    full = X.matrix(ctx)
    lists = _exclusions(X, np.random.default_rng(k))
    ex = _csr(lists)
    idx, sc, cnt = X.topk(ctx, k, ex=ex)
    ties = 0
    for r in range(N_HIST):
        e_idx, e_sc, e_cnt = _expected_topk(full[r], lists[r], k)
        assert np.array_equal(idx[r], e_idx), (r, idx[r], e_idx)
        assert np.array_equal(sc[r].view(np.int32), e_sc.view(np.int32)), r                 # the matrix's bits
        assert cnt[r] == e_cnt == N_ITEM - len(lists[r])
        if r % 3 == 2 and k > 5:
            assert np.all(idx[r][5:] == -1) and np.all(sc[r][5:] == -np.inf) and np.all(idx[r][:5] >= 0)
        ties += int(np.sum((sc[r][1:] == sc[r][:-1]) & (idx[r][1:] > idx[r][:-1]) & (idx[r][:-1] >= 0)))
    if k > 1:
        assert ties > 0                                                                     # the planted copies reach the lists
    # every span gives the same bits; so does a row alone
    for span in (256, 1024, 4096):                                                          # 9, 3 and 1 spans per row
        ctx.set_option("geoie_score_span", span)
        i2, s2, c2 = X.topk(ctx, k, ex=ex)
        assert ctx.last_plan("geoie_score_splits") == -(-N_ITEM // span)
        assert np.array_equal(i2, idx) and np.array_equal(s2.view(np.int32), sc.view(np.int32)) and np.array_equal(c2, cnt), span
        one = X.topk(ctx, k, rows=[13], ex=_csr([lists[13]]))
        assert np.array_equal(one[0][0], idx[13]) and np.array_equal(one[1][0].view(np.int32), sc[13].view(np.int32)) and one[2][0] == cnt[13]
    ctx.set_option("geoie_score_span", 0)
    for r in (0, 5, 7, 13):
        one = X.topk(ctx, k, rows=[r], ex=_csr([lists[r]]))
        assert ctx.last_plan("geoie_score_splits") > 1                                      # one history is still cut into spans
        assert np.array_equal(one[0][0], idx[r]) and np.array_equal(one[1][0].view(np.int32), sc[r].view(np.int32)) and one[2][0] == cnt[r]
    # without lists and without a user term
    i3, s3, c3 = X.topk(ctx, k, with_tu=False)
    bare = X.matrix(ctx, with_tu=False)
    for r in range(N_HIST):
        e_idx, e_sc, e_cnt = _expected_topk(bare[r], [], k)
        assert np.array_equal(i3[r], e_idx) and np.array_equal(s3[r].view(np.int32), e_sc.view(np.int32)) and c3[r] == e_cnt


def test_bad_rows_are_rejected_alone(ctx):
    X = problem(20, 0.7)
    good = [np.array([3, 8, 20]), np.array([1, 2])]
    hs = [good[0], np.array([5, 9, N_ITEM]), np.array([7, 7, 9]), good[1], np.array([9, 4]), np.array([-1, 3]), np.array([6, 30])]
    ms = [np.array([2, 1, 4]), np.ones(3), np.ones(3), np.array([1, 3]), np.ones(2), np.ones(2), np.array([1, 0])]
    bad = [1, 2, 4, 5, 6]
    off, flat = _csr(hs)
    csr = (_i32(off), _i32(flat), _i32(_csr(ms)[1]))
    goff, gflat = _csr(good)
    gcsr = (_i32(goff), _i32(gflat), _i32(_csr([ms[0], ms[3]])[1]))
    rows = np.arange(len(hs))
    ctx.take_bad_ids()
    got = X.matrix(ctx, rows=rows, csr=csr, with_tu=False)
    assert ctx.take_bad_ids() == len(bad)                                                   # each bad row once, whatever its spans
    clean = X.matrix(ctx, rows=[0, 1], csr=gcsr, with_tu=False)
    assert ctx.take_bad_ids() == 0
    assert np.isnan(got[bad]).all() and np.array_equal(got[[0, 3]], clean) and np.isfinite(clean).all()
    want, M = S.scores_geo(X.P, np.repeat(good[0], ms[0]), X.coords, 0.01)
    assert np.all(np.abs(got[0] - want) <= TOL * M)
    idx, sc, cnt = X.topk(ctx, 20, rows=rows, csr=csr, with_tu=False)
    assert ctx.take_bad_ids() == len(bad)
    assert np.all(idx[bad] == -1) and np.all(sc[bad] == -np.inf) and np.all(cnt[bad] == 0)
    for i in (0, 3):
        e_idx, e_sc, e_cnt = _expected_topk(got[i], [], 20)
        assert np.array_equal(idx[i], e_idx) and np.array_equal(sc[i], e_sc) and cnt[i] == e_cnt
    # a malformed exclusion list rejects its row only
    idx, sc, cnt = X.topk(ctx, 20, rows=[0, 3], csr=csr, with_tu=False, ex=(np.array([0, 1, 2]), np.array([N_ITEM, 4])))
    assert ctx.take_bad_ids() == 1 and np.all(idx[0] == -1) and cnt[0] == 0 and cnt[1] == N_ITEM - 1 and 4 not in idx[1]
    # n_rows = 0 is a no-op
    prm = X.prm()
    ctx.check(ctx.lib.poi_geoie_score_all_geo(ctx.handle, ctypes.byref(prm), None, None, None, None, None, 0, None, None, 0.01, None, _stream()))


# ---- model level ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    ds = D.make_synthetic(70, 900, 30, 5)
    m = OboGeoIE(train=ds.shard(), test=None, alpha_lambda=[0.01, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_in=20, n_hidden=20,
                 coords=ds.coords, seed=3, d_min=0.01)
    m.train_batch(np.arange(ds.n_user))
    m.update_trained()
    return ds, m


def test_reference_rule_is_bitwise_what_it_was(ctx, trained):
    ds, m = trained
    assert m.score_rule == "reference" and m._rank_fused
    se = np.arange(5, 60, dtype=np.int32)
    uv = torch.empty((ds.n_user, 40), dtype=torch.float32, device="cuda")
    prm = m._gparams(m._trained)
    ctx.check(ctx.lib.poi_geoie_user_vectors(ctx.handle, ctypes.byref(prm), P_(m.off), P_(m.p), ds.n_user, m.len_max, 0, P_(uv), _stream()))
    items = torch.cat([m._trained["z"], m._trained["h"]], 1).contiguous()
    users = uv[5:60].contiguous()
    out = torch.empty((55, ds.n_item), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.poi_score_all(ctx.handle, P_(users), P_(items), 55, ds.n_item, 40, None, None, P_(out), _stream()))
    idx = torch.empty((55, 20), dtype=torch.int32, device="cuda")
    sc = torch.empty((55, 20), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.poi_score_topk(ctx.handle, P_(users), P_(items), 55, ds.n_item, 40, None, None, 20, P_(idx), P_(sc), _stream()))
    for rule in (None, "reference"):
        assert torch.equal(m.compute_sub_all_scores_device(se, rule), out)
        i2, s2 = m.compute_sub_topk(se, 20, return_scores=True, rule=rule)
        assert torch.equal(i2, idx) and torch.equal(s2, sc)
    assert np.array_equal(m.compute_sub_all_scores(se), out.cpu().numpy())
    with pytest.raises(ValueError):
        m.compute_sub_topk(se, 20, rule="bogus")


def test_model_geo_rule(ctx, trained):
    ds, m = trained
    se = np.arange(5, 60, dtype=np.int32)
    full = m.compute_sub_all_scores(se, rule="geo")
    Pt = {k: m._trained[k].cpu().numpy().astype(np.float64) for k in O.TABLES}
    Pt["a"], Pt["b"] = float(m.a.get_value()), float(m.b.get_value())
    off = np.asarray(ds.off, np.int64)
    for i in (0, 17, 54):
        u = int(se[i])
        want, M = S.scores_geo(Pt, ds.tra_p[off[u]:off[u + 1]], ds.coords, 0.01, Pt["t"][u])
        assert np.all(np.abs(full[i] - want) <= TOL * M), u
    for k in (20, 50):                                                                      # the fused kernel; score rows + poi_topk
        idx, sc = m.compute_sub_topk(se, k, return_scores=True, rule="geo")
        for i in range(len(se)):
            e_idx, e_sc, _ = _expected_topk(full[i], [], k)
            assert np.array_equal(idx[i].cpu().numpy(), e_idx) and np.array_equal(sc[i].cpu().numpy(), e_sc), (k, i)
    eo, ex = (t.cpu().numpy() for t in m.train_exclusion())
    idx, cnt = m.compute_sub_topk(se, 20, rule="geo", exclude="train", return_counts=True)
    for i, u in enumerate(se):
        mine = ex[eo[u]:eo[u + 1]]
        e_idx, _, e_cnt = _expected_topk(full[i], mine, 20)
        assert np.array_equal(idx[i].cpu().numpy(), e_idx) and int(cnt[i]) == e_cnt
    # ranks: under "geo" the instance goes through its score rows and poi_rank_scores
    m.score_rule = "geo"
    try:
        assert not m._rank_fused
        assert np.array_equal(m.compute_sub_all_scores(se), full)
        rank, cnt = m.compute_sub_target_rank(se, exclude="train", return_counts=True)
        want = R.ranks(full, ds.tes_p[se].reshape(-1, 1), np.ones((len(se), 1)), eo[se[0]:se[-1] + 2] - eo[se[0]], ex[eo[se[0]]:])
        assert np.array_equal(rank.cpu().numpy(), want["rank"]) and np.array_equal(cnt.cpu().numpy(), want["count"])
        fm = E.full_rank_metrics(m, harness.compute_start_end(ds.n_user, 32), [5, 20])
        allr = R.ranks(m.compute_sub_all_scores(np.arange(ds.n_user)), ds.tes_p.reshape(-1, 1), np.ones((ds.n_user, 1)))
        assert abs(fm["mrr"] - R.summary(allr["rank"], allr["count"])["mrr"]) <= 1e-12
    finally:
        m.score_rule = "reference"


def test_unseen_users(ctx, trained):
    ds, m = trained
    off = np.asarray(ds.off, np.int64)
    users = np.array([3, 40, 12, 66, 9])
    hist = [ds.tra_p[off[u]:off[u + 1]] for u in users]
    tt = m._trained["t"][torch.as_tensor(users).cuda()]
    # a trained user's own history with its own t row is that user, bit for bit
    own_i, own_s = m.compute_sub_topk(users, 20, return_scores=True, rule="geo")
    new_i, new_s = m.recommend_new(hist, 20, exclude=None, return_scores=True, user_term=tt)
    assert torch.equal(own_i, new_i) and torch.equal(own_s, new_s)
    assert torch.equal(m.score_new(hist, user_term=tt), m.compute_sub_all_scores_device(users, rule="geo"))
    # the unseen user: tu = 0; a history's bits do not depend on the other histories of the call
    mat = m.score_new(hist)
    assert torch.equal(m.score_new([hist[2]]), mat[2:3]) and torch.equal(m.score_new((_csr(hist)[0], _csr(hist)[1])), mat)
    Pt = {k: m._trained[k].cpu().numpy().astype(np.float64) for k in O.TABLES}
    Pt["a"], Pt["b"] = float(m.a.get_value()), float(m.b.get_value())
    want, M = S.scores_geo(Pt, hist[1], ds.coords, 0.01)
    assert np.all(np.abs(mat[1].cpu().numpy() - want) <= TOL * M)
    idx, sc, cnt = m.recommend_new(hist, 20, return_scores=True, return_counts=True)      # exclude = "history"
    matn = mat.cpu().numpy()
    for i in range(len(users)):
        e_idx, e_sc, e_cnt = _expected_topk(matn[i], np.unique(hist[i]), 20)
        assert np.array_equal(idx[i].cpu().numpy(), e_idx) and np.array_equal(sc[i].cpu().numpy(), e_sc) and int(cnt[i]) == e_cnt
    # ranks of the held-out POIs, and the fold-in metrics on the model as it is
    tgt = ds.tes_p[users].reshape(-1, 1)
    rank, cnt = m.rank_new(hist, tgt, return_counts=True)
    eo, ex = _csr([np.unique(h) for h in hist])
    want = R.ranks(matn, tgt, np.ones_like(tgt), eo, ex)
    assert np.array_equal(rank.cpu().numpy(), want["rank"]) and np.array_equal(cnt.cpu().numpy(), want["count"])
    fm = E.foldin_rank_metrics(m, hist, tgt, [5, 20])
    rs = E.rank_summary(want["rank"], want["count"], [5, 20])
    assert abs(fm["mrr"] - rs["mrr"]) <= 1e-12 and fm["at"][20]["hits"] == rs["at"][20]["hits"]
    with pytest.raises(IndexError):
        m.score_new([[1, ds.n_item + 3]])


def test_trained_rule_carries_more_signal_than_the_reference_rule(ctx):
    """The planted problem of tests/geoie_score_oracle.py under test_train_geoie_learns' schedule (4 epochs, launches of 128 users,
    alpha 0.05, d_min 0.01, negatives redrawn per epoch): MRR of the held-out POI among all POIs, same snapshot, both rules.
    Measured on MI355X: MRR 0.2495 under "geo", 0.0086 under "reference" (recall@20 0.598 / 0.025); DESIGN.md section 21."""
    ds, init = S.planted_problem()
    m = OboGeoIE(train=ds.shard(), test=None, alpha_lambda=[0.05, 0.001], n_user=ds.n_user, n_item=ds.n_item, n_in=20, n_hidden=20,
                 coords=ds.coords, init=init, seed=5, d_min=0.01, score_norm="count")
    for epoch in range(4):
        if epoch > 0:
            m.resample_negatives_device(5 * 1000003 + epoch)
        order = np.random.default_rng(123 + epoch).permutation(ds.n_user)
        losses = np.concatenate([m.train_batch(order[s:s + 128]) for s in range(0, ds.n_user, 128)])
        assert np.isfinite(losses).all() and m.rejected == 0
    m.update_trained()
    ses = harness.compute_start_end(ds.n_user, 64)
    ref = E.full_rank_metrics(m, ses, [20])
    m.score_rule = "geo"
    geo = E.full_rank_metrics(m, ses, [20])
    print("MRR geo %.4f reference %.4f  recall@20 geo %.4f reference %.4f  a %.4f b %.4f"
          % (geo["mrr"], ref["mrr"], geo["at"][20]["recall"], ref["at"][20]["recall"], float(m.a.get_value()), float(m.b.get_value())))
    assert geo["mrr"] >= ref["mrr"], (geo["mrr"], ref["mrr"])
