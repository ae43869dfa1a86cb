"""GeoIE, CPU half: the float64 oracle step against torch autograd of the reference's cost as written (public/GeoIE.py:129-188), the
engine's rules for the reference's undefined cases, the host pair distances against the reference's own data path (golden), and the
declarations of the GeoIE entry points (additive to ABI 9)."""
import os
import re

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D
from tests import geoie_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coords(rng, n_item):
    return np.stack([40 + 0.3 * rng.random(n_item), -74 + 0.4 * rng.random(n_item)], 1)


def _autograd(P, u, p, q, coords, alpha, lam):
    """The reference's graph on the valid pairs: gps, hps, hqs, zps, zqs gathered, sp / sq with t_z, cost = -loss + 0.5 lambda sum of
    squares of the gathered rows; every table and a, b move by -alpha d cost / d (.)."""
    import torch
    T = {k: torch.tensor(P[k], dtype=torch.float64, requires_grad=True) for k in O.TABLES}
    a = torch.tensor(P["a"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(P["b"], dtype=torch.float64, requires_grad=True)
    R = len(p) - 1
    dp, dq = O.pair_dists(coords, p, q)
    M = torch.tensor(np.tril(np.ones((R, R))), dtype=torch.float64)
    dpt = torch.where(M > 0, torch.tensor(dp, dtype=torch.float64), torch.ones(R, R, dtype=torch.float64))
    dqt = torch.where(M > 0, torch.tensor(dq, dtype=torch.float64), torch.ones(R, R, dtype=torch.float64))
    pi, qi = torch.tensor(p), torch.tensor(q)
    gps, hps, hqs = T["g"][pi[:R]], T["h"][pi[1:]], T["h"][qi[1:]]
    zps, zqs, tu = T["z"][pi[1:]], T["z"][qi[1:]], T["t"][u]
    t_z = (tu * zps).sum(1)
    n_h = M.sum(1)
    eg = gps.reshape(1, R, -1) * M.reshape(R, R, 1)
    sp = ((eg * hps.reshape(R, 1, -1)).sum(2) * (a * dpt ** b) * M).sum(1) / n_h + t_z
    sq = ((eg * hqs.reshape(R, 1, -1)).sum(2) * (a * dqt ** b) * M).sum(1) / n_h + t_z
    loss = torch.log(torch.sigmoid(sp - sq)).sum()
    cost = -loss + 0.5 * lam * sum((x ** 2).sum() for x in (gps, hps, hqs, zps, zqs))
    cost.backward()
    out = {k: (T[k] - alpha * T[k].grad).detach().numpy() for k in O.TABLES}
    out["a"] = float((a - alpha * a.grad).detach())
    out["b"] = float((b - alpha * b.grad).detach())
    return out, float(loss)


@pytest.mark.parametrize("L,dim,b", [(2, 4, 0.3), (7, 8, -0.2), (15, 20, 0.45)])
def test_oracle_step_equals_autograd(L, dim, b):
    rng = np.random.default_rng(L)
    n_item = 24
    P = O.init_tables(rng, 3, n_item, dim)
    P["b"] = b
    coords = _coords(rng, n_item)
    p = rng.permutation(n_item)[:L]                 # no zero distance: the reference is defined everywhere
    q = rng.integers(0, n_item, L)
    for i in range(1, L):
        while q[i] in p[:i]:
            q[i] = rng.integers(0, n_item)
    Q, loss = O.step(P, p, q, coords, 0.01, 0.001)
    R_, los = _autograd(P, 1, p, q, coords, 0.01, 0.001)
    assert abs(loss - los) <= 1e-12 * max(1.0, abs(los))
    for k in O.TABLES:
        np.testing.assert_allclose(Q[k], R_[k], rtol=0, atol=1e-13)
    assert abs(Q["a"] - R_["a"]) <= 1e-13 and abs(Q["b"] - R_["b"]) <= 1e-13
    np.testing.assert_array_equal(Q["t"], P["t"])                                          # t never moves


def test_d_min_zero_distance_and_rejection_rules():
    rng = np.random.default_rng(2)
    n_item, dim = 10, 8
    P = O.init_tables(rng, 2, n_item, dim)
    coords = _coords(rng, n_item)
    p = np.array([1, 2, 1, 3, 4])                                                          # revisit: d(p_2, p_0) = 0
    q = np.array([0, 5, 6, 7, 8])
    # b > 0: the zero-distance pair contributes f = 0, df/db = 0
    P["b"] = 0.3
    Q, loss = O.step(P, p, q, coords, 0.01, 0.001)
    assert np.isfinite(loss)
    # b <= 0 with d_min = 0: rejected (moves nothing, NaN loss); with d_min > 0 defined again
    for bb in (0.0, -0.3):
        P["b"] = bb
        Q, loss = O.step(P, p, q, coords, 0.01, 0.001)
        assert np.isnan(loss) and all(np.array_equal(Q[k], P[k]) for k in O.TABLES) and Q["a"] == P["a"] and Q["b"] == P["b"]
        Q, loss = O.step(P, p, q, coords, 0.01, 0.001, d_min=0.01)
        assert np.isfinite(loss) and not np.array_equal(Q["g"], P["g"])
    # d_min only lifts distances below it: with every distance above, it changes nothing
    P["b"] = 0.2
    p2 = np.array([1, 2, 3, 4])
    Q1, l1 = O.step(P, p2, q[:4], coords, 0.01, 0.001)
    Q2, l2 = O.step(P, p2, q[:4], coords, 0.01, 0.001, d_min=1e-6)
    assert l1 == l2 and all(np.array_equal(Q1[k], Q2[k]) for k in O.TABLES)
    # an id out of range rejects; L < 2 has no rows, loss 0, is not counted for a, b
    Qb, lb = O.batch_step(P, [(np.array([1, n_item]), np.array([0, 2])), (np.array([3]), np.array([4]))], coords, 0.01, 0.001)
    assert np.isnan(lb[0]) and lb[1] == 0.0 and all(np.array_equal(Qb[k], P[k]) for k in O.TABLES) and Qb["a"] == P["a"]
    # z by decay only, t untouched
    Q, _ = O.step(P, p2, q[:4], coords, 0.01, 0.001)
    for r in set(p2[1:].tolist()) | set(q[1:4].tolist()):
        mult = int((p2[1:] == r).sum() + (q[1:4] == r).sum())
        np.testing.assert_allclose(Q["z"][r], P["z"][r] * (1 - 0.01 * 0.001 * mult), rtol=1e-14)
    np.testing.assert_array_equal(Q["t"], P["t"])


def test_batch_rule_of_one_user_is_the_step_and_caps():
    rng = np.random.default_rng(4)
    n_item, dim = 9, 4
    P = O.init_tables(rng, 2, n_item, dim)
    P["b"] = 0.25
    coords = _coords(rng, n_item)
    s = (np.array([0, 1, 2, 3]), np.array([5, 6, 7, 8]))
    Q1, _ = O.step(P, *s, coords, 0.01, 0.001)
    Q2, _ = O.batch_step(P, [s, s], coords, 0.01, 0.001, cap=1.0)                           # the mean of two identical updates
    Q3, _ = O.batch_step(P, [s, s], coords, 0.01, 0.001, cap=1e9)                           # their sum
    for k in ("g", "h", "z"):
        np.testing.assert_allclose(Q2[k], Q1[k], rtol=1e-14, atol=1e-16)
        np.testing.assert_allclose(Q3[k] - P[k], 2 * (Q1[k] - P[k]), rtol=1e-12, atol=1e-16)
    assert np.isclose(Q3["a"] - P["a"], 2 * (Q1["a"] - P["a"]), rtol=1e-12)


def test_user_vectors_and_l2():
    rng = np.random.default_rng(5)
    P = O.init_tables(rng, 3, 6, 4)
    off, p = np.array([0, 2, 2, 5]), np.array([1, 4, 0, 2, 5])
    ref = O.user_vectors(P, off, p, len_max=3, norm="reference")
    cnt = O.user_vectors(P, off, p, len_max=3, norm="count")
    np.testing.assert_allclose(ref[0, 4:], (P["g"][1] + P["g"][4]) / (1 + 4 + 1 * 6))
    np.testing.assert_allclose(cnt[2, 4:], P["g"][[0, 2, 5]].sum(0) / 3)
    assert np.all(cnt[1, 4:] == 0) and np.all(ref[1, 4:] == 0)
    np.testing.assert_array_equal(ref[:, :4], P["t"])
    assert np.isclose(O.l2(P, 0.001), 0.0005 * (sum((P[k] ** 2).sum() for k in O.TABLES) + P["a"] ** 2 + P["b"] ** 2))


# ---- host pair distances against the reference's load_data + fun_compute_dist_neg (tests/golden/make_golden_geoie.py) -------------
@pytest.mark.parametrize("case,split", [("s1", -1), ("s2", -2)])
def test_host_pair_distances_equal_reference_golden(golden_dir, case, split):
    g = np.load(os.path.join(golden_dir, "geoie_pairs.npz"))
    G = lambda k: g[case + "_" + k]
    ds, alias = D.load_sequence_file(os.path.join(golden_dir, "sequences_small.txt"), split=split, seed=1, return_aliases=True)
    assert ds.n_user == int(G("n_user")) and ds.n_item == int(G("n_item"))
    ours = np.array([alias[str(r)] for r in G("ref_ids")] + [ds.n_item])                   # reference alias k -> ours; pad -> pad
    np.testing.assert_array_equal(ds.coords[ours[:-1]], G("cordi"))
    msk = G("tra_masks").astype(bool)
    np.testing.assert_array_equal(ds.lens, msk.sum(1))
    np.testing.assert_array_equal(ds.tra_p, ours[G("tra_buys")][msk])
    q = ours[G("tra_neg")][msk]                                                             # the reference's own negatives
    dp, dq, _, _ = D.geoie_pair_distances(ds.coords, ds.off, ds.tra_p, q)
    np.testing.assert_allclose(dp, G("dp").astype(np.float32), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(dq, G("dq").astype(np.float32), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(D.geoie_pair_distances(ds.coords, ds.off, ds.tra_p, q)[0].astype(np.float64), G("dp"), rtol=1e-6)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_geoie_declarations_match_signatures():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert poi_amd._lib.ABI_VERSION == 9 and re.search(r"#define POI_ABI_VERSION 9\b", hdr)
    assert re.search(r"typedef struct poi_geoie_params \{\s*float\* g; float\* h; float\* t; float\* z; double\* ab;\s*"
                     r"int32_t n_user; int32_t n_item; int32_t dim;", hdr)
    assert [f[0] for f in poi_amd._lib.GeoieParams._fields_] == ["g", "h", "t", "z", "ab", "n_user", "n_item", "dim"]
    for name, nargs in (("poi_geoie_step", 15), ("poi_geoie_pair_distances", 15), ("poi_geoie_user_vectors", 9)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(poi_amd._lib.SIGNATURES[name][1]), name
    i = hdr.index("---- GeoIE (additive to ABI 9)")
    assert i < hdr.index("---- multi-GPU")
    block = hdr[i:hdr.index("---- multi-GPU", i)]
    for s in ("GeoIE.py", "Load_Data_GeoIE.py", '"geoie_row"', '"geoie_col"', '"geoie_sort"', '"geoie_commit"', '"geoie_pairs"',
              '"geoie_uvec"'):
        assert s in block, s
