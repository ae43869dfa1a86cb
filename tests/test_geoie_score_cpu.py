"""GeoIE's trained score rule, CPU half: the oracle of tests/geoie_score_oracle.py against the literal per-occurrence loop and against the
forward values of the training oracle (the rule that is scored is the rule that is trained), the planted problem of the GPU signal test,
and the declarations of the new entry points (additive to ABI 9)."""
import os
import re

import numpy as np
import pytest

import poi_amd
from tests import geoie_oracle as O
from tests import geoie_score_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coords(rng, n_item):
    return np.stack([40 + 0.3 * rng.random(n_item), -74 + 0.4 * rng.random(n_item)], 1)


@pytest.mark.parametrize("b,d_min", [(0.4, 0.0), (-0.6, 0.01), (-0.6, 0.0), (0.0, 0.0)])
def test_oracle_equals_the_literal_double_loop(b, d_min):
    rng = np.random.default_rng(3)
    n_item, dim = 40, 8
    P = O.round_f32(O.init_tables(rng, 2, n_item, dim))
    P["b"] = b
    coords = _coords(rng, n_item)
    coords[7] = coords[3]                                                                   # two POIs at one place
    tu = P["t"][1]
    for hist in ([], [5], [3, 9, 3, 3, 12, 9, 30], list(rng.integers(0, n_item, 25))):
        for t in (None, tu):
            got, M = S.scores_geo(P, hist, coords, d_min, t)
            want = S.scores_geo_literal(P, hist, coords, d_min, t)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=1e-12)
            assert np.all(M[ok] >= np.abs(got[ok]) - 1e-12)
            if not b > 0 and d_min == 0.0 and len(hist):                                       # NaN exactly at the history's places
                at = np.isin(np.arange(n_item), hist) | (np.isin(3, hist) & (np.arange(n_item) == 7))
                assert np.array_equal(np.isnan(got), at)
            else:
                assert ok.all()


@pytest.mark.parametrize("b,d_min,revisit", [(0.3, 0.0, True), (-0.35, 0.01, True), (-0.2, 0.0, False)])
def test_scored_rule_is_the_trained_rule(b, d_min, revisit):
    """Row i of a training user: sp_i = scores_geo(history[:i + 1], tu = t[u])[p_{i+1}], and sq_i the same history at q_{i+1} plus the
    SAME user term t[u].z[p_{i+1}] (GeoIE.py:175-176) - against the forward values of geoie_oracle.user_grads (its pair distances, f, the
    dot products, the 1 / (i + 1) and the loss)."""
    rng = np.random.default_rng(11)
    n_item, dim, L = 60, 12, 18
    P = O.round_f32(O.init_tables(rng, 3, n_item, dim))
    P["b"] = b
    coords = _coords(rng, n_item)
    p = rng.integers(0, n_item, L) if revisit else rng.permutation(n_item)[:L]
    if revisit:
        p[5], p[9] = p[2], p[2]
    q = rng.integers(0, n_item, L)
    for i in range(L):
        while q[i] in set(p.tolist()):
            q[i] = rng.integers(0, n_item)
    u, R = 1, L - 1
    # the forward values as the training oracle derives them
    dp, dq = O.pair_dists(coords, p, q)
    M = np.tril(np.ones((R, R), bool))
    Fp, _, _, badp = O._f(dp, P["a"], b, d_min, M)
    Fq, _, _, badq = O._f(dq, P["a"], b, d_min, M)
    assert not badp and not badq
    Gp, HP, HQ = P["g"][p[:R]], P["h"][p[1:]], P["h"][q[1:]]
    n_h = np.arange(1, R + 1, dtype=np.float64)
    tz = P["z"][p[1:]] @ P["t"][u]
    sp = ((HP @ Gp.T) * Fp).sum(1) / n_h + tz
    sq = ((HQ @ Gp.T) * Fq).sum(1) / n_h + tz
    for i in range(R):
        got, _ = S.scores_geo(P, p[:i + 1], coords, d_min, P["t"][u])
        bare, _ = S.scores_geo(P, p[:i + 1], coords, d_min)
        assert abs(got[p[i + 1]] - sp[i]) <= 1e-12 * max(1.0, abs(sp[i])), i
        assert abs(bare[q[i + 1]] + tz[i] - sq[i]) <= 1e-12 * max(1.0, abs(sq[i])), i
    diff = sp - sq
    assert abs(float(-np.logaddexp(0.0, -diff).sum()) - O.user_grads(P, p, q, coords, d_min)["loss"]) <= 1e-10


def _mrr(score_rows, targets):
    r = [int(((s > s[t]) | ((s == s[t]) & (np.arange(len(s)) < t))).sum()) for s, t in zip(score_rows, targets)]
    return float(np.mean(1.0 / (np.asarray(r) + 1.0)))


def test_planted_problem_orders_the_rules_on_the_oracle_side():
    """Before any training the planted tables already rank the held-out POI higher under the trained rule than under the reference rule
    (float64 oracles on a slice of the users): the ordering the GPU test asserts after training is a property of the data."""
    ds, init = S.planted_problem()
    P = O.round_f32(init)
    off = np.asarray(ds.off, np.int64)
    users = np.arange(0, ds.n_user, 6)
    uv = O.user_vectors(P, ds.off, ds.tra_p, int(np.diff(off).max()), "count")
    ref = O.scores(P, uv[users])
    geo = [np.nan_to_num(S.scores_geo(P, ds.tra_p[off[u]:off[u + 1]], ds.coords, 0.01, P["t"][u])[0], nan=-np.inf) for u in users]
    tgt = np.asarray(ds.tes_p).reshape(ds.n_user, -1)[users, 0]
    m_geo, m_ref = _mrr(geo, tgt), _mrr(ref, tgt)
    assert m_geo > 2 * m_ref, (m_geo, m_ref)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_geo_score_declarations_match_signatures():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert poi_amd._lib.ABI_VERSION == 9 and re.search(r"#define POI_ABI_VERSION 9\b", hdr)
    assert re.search(r"/\* additive to 9: GeoIE scoring under the trained geo-influence law", hdr[:hdr.index("#define POI_ABI_VERSION")])
    for name, nargs in (("poi_geoie_score_all_geo", 13), ("poi_geoie_score_topk_geo", 18)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(poi_amd._lib.SIGNATURES[name][1]), name
    block = hdr[hdr.index("---- GeoIE (additive to ABI 9)"):hdr.index("---- POI2Vec (additive to ABI 9)")]
    for s in ('"geoie_score_geo"', '"geoie_topk_geo"', '"geoie_score_span"', '"geoie_score_splits"', "strictly ascending", "DESIGN.md section 21"):
        assert s in block, s
    assert "geoie_score.hip" in poi_amd.build.SOURCES and "geoie_pair.h" in poi_amd.build.HEADERS
    csrc = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "geoie_score.hip")) and os.path.exists(os.path.join(csrc, "geoie_pair.h"))
    for k in ("geoie_score_span", "geoie_score_splits"):
        assert k in poi_amd._lib.PLAN_KEYS
    abi = open(os.path.join(csrc, "abi.hip")).read()
    assert '{"geoie_score_span", &c->geo_span' in abi and '"geoie_score_splits"' in abi[abi.index("int poi_ctx_last_plan("):]
    # one definition of the pair math: the step includes it, it does not copy it
    step = open(os.path.join(csrc, "geoie.hip")).read()
    assert '#include "geoie_pair.h"' in step and "float gi_dist(" not in step and "void gi_f(" not in step


def test_library_exports_the_entries():
    lib = poi_amd._lib.load()
    assert hasattr(lib, "poi_geoie_score_all_geo") and hasattr(lib, "poi_geoie_score_topk_geo")


def test_bogus_score_rule_raises():
    from poi_amd.models import OboGeoIE
    with pytest.raises(ValueError, match="score_rule"):
        OboGeoIE(train=[[[0, 1]], [[1, 1]], [[1, 0]], [[1, 1]]], test=[[[1]], [[1]]], alpha_lambda=[0.01, 0.001], n_user=1, n_item=2, n_in=4,
                 n_hidden=4, coords=np.zeros((2, 2)), score_rule="bogus")
