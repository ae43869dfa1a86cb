"""CPU checks of the VBPR oracle (tests/vbpr_oracle.py) and of the feature's public surface: the oracle's single step against torch
autograd of the literal cost of public/BPR.py:287-308, the batch rule at n == 1 against the single step, and the header / package
declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

from tests import vbpr_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed, n_user=7, n_item=12, d=8, f=36, scale=1.0):
    rng = np.random.default_rng(seed)
    P = V.init_params(rng, n_user, n_item, d, f)
    fi = np.zeros((n_item + 1, f))
    fi[:n_item] = np.maximum(rng.standard_normal((n_item, f)), 0.0) * scale
    return P, fi


@pytest.mark.parametrize("seed,scale", [(1, 1.0), (2, 1.0 / 6.0), (3, 0.05)])
def test_oracle_step_matches_autograd_of_the_literal_cost(seed, scale):
    torch = pytest.importorskip("torch")
    P, fi = _problem(seed, scale=scale)
    alpha, lam, lam_ev = 0.01, 0.001, 0.002
    u, p, q = 3, 5, 9
    T = {k: torch.tensor(P[k], dtype=torch.float64, requires_grad=True) for k in V.NAMES}
    F = torch.tensor(fi, dtype=torch.float64)
    usr, xp, xq, use = T["ux"][u], T["lt"][p], T["lt"][q], T["ue"][u]
    uij = torch.dot(usr, xp - xq) + torch.dot(use, T["ei"] @ (F[p] - F[q]))                      # :287-289
    upq = torch.log(torch.sigmoid(uij))
    cost = -upq + 0.5 * lam * ((usr ** 2).sum() + (xp ** 2).sum() + (xq ** 2).sum() + (use ** 2).sum()) + 0.5 * lam_ev * (T["ei"] ** 2).sum()
    cost.backward()
    N, loss = V.step(P, fi, u, p, q, alpha, lam, lam_ev)
    for k in V.NAMES:
        want = P[k] - alpha * T[k].grad.numpy()
        assert np.abs(N[k] - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), k
    assert abs(loss - float(-upq.detach())) <= 1e-10 * max(1.0, abs(loss))


@pytest.mark.parametrize("cap", [1.0, 8.0, 1e9])
def test_batch_rule_at_n1_is_the_single_step(cap):
    P, fi = _problem(4)
    N1, l1 = V.step(P, fi, 2, 0, 7, 0.01, 0.001, 0.002)
    NB, lb = V.batch_step(P, fi, [2], [0], [7], 0.01, 0.001, 0.002, cap)
    for k in V.NAMES:
        assert np.abs(N1[k] - NB[k]).max() <= 1e-14, k
    assert abs(l1 - lb[0]) <= 1e-14


def test_batch_rule_rejects_and_caps():
    P, fi = _problem(5)
    u, p, q = np.array([1, 1, 7, 2, 3]), np.array([0, 2, 1, 4, 13]), np.array([3, 5, 2, 4, 1])      # user 7 / p == q / POI 13: rejected
    N, loss = V.batch_step(P, fi, u, p, q, 0.01, 0.001, 0.002, 1.0)
    M, lm = V.batch_step(P, fi, u[:2], p[:2], q[:2], 0.01, 0.001, 0.002, 1.0)
    assert np.isnan(loss[2:]).all() and np.array_equal(loss[:2], lm)
    assert all(np.array_equal(N[k], M[k]) for k in V.NAMES)
    # cap 1: the shared user row moves by the MEAN of its two single steps
    a, _ = V.step(P, fi, 1, 0, 3, 0.01, 0.001, 0.002); b, _ = V.step(P, fi, 1, 2, 5, 0.01, 0.001, 0.002)
    assert np.abs(N["ux"][1] - 0.5 * (a["ux"][1] + b["ux"][1])).max() <= 1e-14
    assert np.abs(N["ei"] - 0.5 * (a["ei"] + b["ei"])).max() <= 1e-14


def test_snapshots_and_l2():
    P, fi = _problem(6)
    it, us = V.items(P, fi), V.users(P)
    assert it.shape == (13, 16) and us.shape == (7, 16)
    assert np.array_equal(it[:, :8], P["lt"]) and np.abs(it[12, 8:]).max() == 0.0      # pad row: zero features
    want = 0.5 * 0.001 * sum((P[k] ** 2).sum() for k in ("ux", "lt", "ue")) + 0.5 * 0.002 * (P["ei"] ** 2).sum()
    assert abs(V.l2(P, 0.001, 0.002) - want) <= 1e-12


def test_header_declares_the_vbpr_entries_and_the_package_has_the_model():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    for sym in ("poi_vbpr_params", "poi_vbpr_step", "poi_vbpr_items", "poi_vbpr_users"):
        assert re.search(r"\b%s\b" % sym, hdr), sym
    assert re.search(r"#define\s+POI_ABI_VERSION\s+9\b", hdr)
    import poi_amd
    assert poi_amd._lib.ABI_VERSION == 9
    assert hasattr(poi_amd.models, "OboVBpr") and issubclass(poi_amd.models.OboVBpr, poi_amd.models.MfBasic)
    for sym in ("poi_vbpr_step", "poi_vbpr_items", "poi_vbpr_users"):
        assert sym in poi_amd._lib.SIGNATURES
    f = poi_amd.data.synthetic_features(9, 36, 1)
    assert f.shape == (10, 36) and f.dtype == np.float32 and (f >= 0).all() and not f[9].any() and f[:9].any()
