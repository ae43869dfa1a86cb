"""PRME, CPU half: the float64 oracle step against torch autograd of the reference graph (public/PRME.py:173-214, with set_subtensor's
last-wins assignment), the loader against the reference's own load_data (golden), and the ABI 8 declarations."""
import os
import re

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D
from tests import prme_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd_step(P, u, p, q, prev, d, gap, alpha, lam, thd=360, cw=0.2):
    """Gather du[u], dp[[p, q, prev]], ds[[p, q, prev]]; cost = log sigmoid(Dq - Dp) - 1/2 lambda sum of squares of the gathered rows;
    each gathered row -> row + alpha d cost / d row, assigned in order so that the last occurrence of a repeated index wins."""
    import torch
    T = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
    du = T["du"][u].clone().requires_grad_()
    dp = T["dp"][[p, q, prev]].clone().requires_grad_()
    ds = T["ds"][[p, q, prev]].clone().requires_grad_()
    w = (1.0 + d) ** 0.25
    Dp_p, Dp_q = ((du - dp[0]) ** 2).sum(), ((du - dp[1]) ** 2).sum()
    Ds_p, Ds_q = ((ds[0] - ds[2]) ** 2).sum(), ((ds[1] - ds[2]) ** 2).sum()
    if gap > thd:
        Dp, Dq = Dp_p, Dp_q
    else:
        Dp, Dq = w * (cw * Dp_p + (1 - cw) * Ds_p), w * (cw * Dp_q + (1 - cw) * Ds_q)
    upq = torch.log(torch.sigmoid(Dq - Dp))
    cost = upq - 0.5 * lam * sum((x ** 2).sum() for x in (du, dp, ds))
    cost.backward()
    out = {k: v.clone() for k, v in T.items()}
    out["du"][u] = du + alpha * du.grad
    for k, sub in (("dp", dp), ("ds", ds)):
        new = sub + alpha * sub.grad
        for r, idx in enumerate((p, q, prev)):
            out[k][idx] = new[r]
    return {k: v.detach().numpy() for k, v in out.items()}, float(upq.detach())


@pytest.mark.parametrize("case", ["near", "far", "p_eq_prev", "q_eq_prev", "near_dim64"])
def test_oracle_step_equals_autograd(case):
    rng = np.random.default_rng(11)
    dim = 64 if case == "near_dim64" else 20
    P = O.init_tables(rng, 5, 30, dim)
    u, p, q, prev, d, gap = 3, 11, 4, 17, 2.75, 120
    if case == "far":
        gap = 361
    if case == "p_eq_prev":
        prev = p
    if case == "q_eq_prev":
        prev = q
    Q, loss = O.step(P, u, p, q, prev, d, gap, 0.01, 0.001)
    R, los = _autograd_step(P, u, p, q, prev, d, gap, 0.01, 0.001)
    assert abs(loss - los) <= 1e-13 * max(1.0, abs(los))
    for k in O.TABLES:
        np.testing.assert_allclose(Q[k], R[k], rtol=0, atol=1e-14)
    if case == "p_eq_prev":             # dp[p] by decay only, ds[p] takes the prev occurrence's update
        np.testing.assert_allclose(Q["dp"][p], P["dp"][p] * (1 - 0.01 * 0.001), rtol=1e-14)
        assert not np.allclose(Q["ds"][p], P["ds"][p] * (1 - 0.01 * 0.001))
    if case == "far":                   # every ds row by decay only
        for r in (p, q, prev):
            np.testing.assert_allclose(Q["ds"][r], P["ds"][r] * (1 - 0.01 * 0.001), rtol=1e-14)


def test_batch_rule_of_one_transition_is_the_step_and_rejects_bad_ones():
    rng = np.random.default_rng(3)
    P = O.init_tables(rng, 4, 12, 8)
    Q1, l1 = O.step(P, 1, 2, 3, 5, 0.5, 10, 0.01, 0.001)
    Qb, lb = O.batch_step(P, [1], [2], [3], [5], [0.5], [10], 0.01, 0.001, cap=1.0)
    assert np.isclose(lb[0], l1) and all(np.array_equal(Q1[k], Qb[k]) for k in O.TABLES)
    bad = dict(u=[9, 2, 3, 5, 0.5], p=[1, 13, 3, 5, 0.5], pq=[1, 3, 3, 5, 0.5], dn=[1, 2, 3, 5, np.nan], dneg=[1, 2, 3, 5, -1.0],
               dinf=[1, 2, 3, 5, np.inf])
    for name, (u, p, q, v, d) in bad.items():
        Qb, lb = O.batch_step(P, [u], [p], [q], [v], [d], [10], 0.01, 0.001)
        assert np.isnan(lb).all() and all(np.array_equal(Qb[k], P[k]) for k in O.TABLES), name


def test_score_rows_and_reference_layout():
    rng = np.random.default_rng(4)
    P = O.init_tables(rng, 3, 6, 4)
    coords = np.vstack([np.stack([40 + rng.random(6), -74 + rng.random(6)], 1), [[0.0, 0.0]]])
    sc = O.score_rows(P, coords, [0, 2], [1, 6])
    j = 4
    w = (1 + O.cal_dis(coords[1, 0], coords[1, 1], coords[j, 0], coords[j, 1])) ** 0.25
    ref = -w * (0.2 * ((P["du"][0] - P["dp"][j]) ** 2).sum() + 0.8 * ((P["ds"][1] - P["ds"][j]) ** 2).sum())
    assert sc.shape == (2, 6) and np.isclose(sc[0, j], ref, rtol=1e-14)
    off = np.array([0, 2, 5, 6]); tra = np.array([0, 1, 2, 3, 4, 5])
    tes = np.array([[1, 2, 6], [3, 6, 6], [0, 1, 2]]); msk = (tes < 6).astype(int)
    users, qpoi, lb = O.reference_rows(off, tra, tes, msk, np.array([0, 1]), 6)
    assert lb == 2 and users.tolist() == [0, 0, 1, 1] and qpoi.tolist() == [1, 1, 4, 3]
    assert np.isclose(O.l2(P, 0.001), 0.0005 * sum((P[k] ** 2).sum() for k in O.TABLES))


# ---- loader against the reference's load_data + fun_data_pois_masks (tests/golden/make_golden_prme.py) ----------------------------
@pytest.mark.parametrize("mode", ["test", "valid"])
def test_loader_equals_reference_golden(golden_dir, mode):
    g = np.load(os.path.join(golden_dir, "prme_load_data.npz"))
    path = os.path.join(golden_dir, "sequences_small.txt" if mode == "test" else "prme_valid_small.txt")
    split = (0.8, 1.0) if mode == "test" else (0.6, 0.8)
    ds, alias = D.load_prme_sequence_file(path, split=split, seed=1, return_aliases=True)
    G = lambda k: g[mode + "_" + k]
    assert ds.n_user == int(G("n_user")) and ds.n_item == int(G("n_item"))
    ours = np.array([alias[str(r)] for r in G("ref_ids")] + [ds.n_item])        # reference alias k -> ours; pad -> pad
    assert len(set(ours.tolist())) == ds.n_item + 1
    np.testing.assert_array_equal(ds.coords[ours], G("location"))               # last-occurrence coordinates + the (0, 0) pad row
    msk = G("tra_masks").astype(bool)
    np.testing.assert_array_equal(ds.lens, msk.sum(1))
    np.testing.assert_array_equal(ds.tra_p, ours[G("tra_pois")][msk])
    np.testing.assert_array_equal(ds.tra_gap, G("tra_times")[msk].astype(np.int64))
    np.testing.assert_allclose(ds.tra_d, G("tra_dists")[msk], rtol=1e-13, atol=1e-12)
    np.testing.assert_array_equal(ds.tes_mask, G("tes_masks"))
    np.testing.assert_array_equal(ds.tes_p, ours[G("tes_pois")])
    # negatives: the rules of fun_random_neg_masks_tra / _tes
    assert ds.tra_q.shape == ds.tra_p.shape and ds.tes_q.shape == ds.tes_p.shape
    off = np.asarray(ds.off, np.int64)
    for u in range(ds.n_user):
        own = set(ds.tra_p[off[u]:off[u + 1]].tolist())
        tes = set(ds.tes_p[u][ds.tes_mask[u] > 0].tolist())
        assert not own & set(ds.tra_q[off[u]:off[u + 1]].tolist())
        tq = ds.tes_q[u]
        assert np.all(tq[ds.tes_mask[u] == 0] == ds.n_item) and not (own | tes) & set(tq[ds.tes_mask[u] > 0].tolist())


def test_loader_raises_like_the_reference_on_a_dropped_only_poi(golden_dir):
    g = np.load(os.path.join(golden_dir, "prme_load_data.npz"))
    assert int(g["valid_small_raises"]) == 1
    with pytest.raises(KeyError):
        D.load_prme_sequence_file(os.path.join(golden_dir, "sequences_small.txt"), split=(0.6, 0.8))


def test_loader_rejects_fractional_gaps(tmp_path):
    p = tmp_path / "s.txt"
    p.write_text("check_times pois_different u_id u_pois u_times u_coordinates\n"
                 "3 1.0 0 1/2/3 0/1.5/3 40.0,-74.0/40.01,-74.0/40.02,-74.0\n")
    with pytest.raises(ValueError):
        D.load_prme_sequence_file(str(p))


def test_synthetic_builder_gap_fraction():
    ds = D.make_prme_synthetic(300, 500, 20, 7, far_frac=0.4)
    first = np.zeros(len(ds.tra_p), bool)
    first[np.asarray(ds.off[:-1], np.int64)] = True
    frac = float((ds.tra_gap[~first] > 360).mean())
    assert 0.3 < frac < 0.5 and np.all(ds.tra_gap[first] == 0) and np.all(ds.tra_d[first] == 0)
    assert ds.coords.shape == (ds.n_item + 1, 2) and np.all(ds.coords[-1] == 0)


# ---- ABI 8 entries (unchanged in ABI 9) --------------------------------------------------------------------------------------------
def test_abi8_declarations_match_signatures_in_abi9():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert poi_amd._lib.ABI_VERSION == 9 and re.search(r"#define POI_ABI_VERSION 9\b", hdr)
    assert re.search(r"typedef struct poi_prme_params \{\s*float\* du; float\* dp; float\* ds;\s*int32_t n_user; int32_t n_item; int32_t dim;", hdr)
    assert [f[0] for f in poi_amd._lib.PrmeParams._fields_] == ["du", "dp", "ds", "n_user", "n_item", "dim"]
    for name, nargs in (("poi_prme_step", 15), ("poi_prme_score_all", 9), ("poi_prme_score_topk", 11)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(poi_amd._lib.SIGNATURES[name][1]), name
    # every new entry cites the reference and names its timings
    i = hdr.index("---- PRME (ABI 8)")
    block = hdr[i:hdr.index("---- multi-GPU", i)]
    for s in ("PRME.py", "Load_Data_prme.py", '"prme_fwd"', '"prme_sort"', '"prme_rows"', '"prme_commit"', '"prme_score_all"', '"prme_score_topk"'):
        assert s in block, s
