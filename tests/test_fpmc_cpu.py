"""FPMC-LR, CPU half: the host neighbour sets against the reference's own (golden), the neighbour threshold against scalar libm, and the
float64 oracle step against torch autograd of the written-out cost (public/FPMC_LR.py:113-151)."""
import math
import os

import numpy as np
import pytest

from poi_amd import data as D
from tests import fpmc_oracle as F


@pytest.mark.parametrize("name", ["small", "hard"])
def test_host_neighbors_equal_reference_golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "fpmc_neighbors.npz"))
    off, ids = D.fpmc_neighbors_host(g[name + "_coords"], float(g["ud_km"]))
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert np.array_equal(off, g[name + "_off"])
    assert np.array_equal(ids, g[name + "_ids"])
    i = np.repeat(np.arange(len(off) - 1), np.diff(off))
    assert not np.any(ids == i)                                     # never the POI itself


def test_hard_golden_set_reaches_the_boundary(golden_dir):
    """The 'hard' set holds pairs whose c is within 1e-10 (relative) of the threshold, on both sides."""
    g = np.load(os.path.join(golden_dir, "fpmc_neighbors.npz"))
    xy = g["hard_coords"]
    c_ud = D.ud_threshold(float(g["ud_km"]))
    cp = D.cos_lat(xy)
    a = (xy[:, 0][:, None] - xy[:, 0][None, :]) * D.DEG
    b = (xy[:, 1][:, None] - xy[:, 1][None, :]) * D.DEG
    c = (1.0 - np.cos(a)) / 2 + cp[:, None] * cp[None, :] * (1.0 - np.cos(b)) / 2
    near = np.abs(c - c_ud) <= 1e-10 * c_ud
    assert (near & (c < c_ud)).sum() >= 50 and (near & (c >= c_ud)).sum() >= 50


@pytest.mark.parametrize("ud", [20.0, 10.0, 1.5, 0.2])
def test_ud_threshold_decides_like_scalar_libm(ud):
    c_ud = D.ud_threshold(ud)
    dist = lambda c: 12742 * math.asin(math.sqrt(c))
    assert dist(c_ud) > ud and dist(np.nextafter(c_ud, 0)) <= ud
    cs = [c_ud]
    for _ in range(40):
        cs.append(np.nextafter(cs[-1], 1.0))
        cs.insert(0, np.nextafter(cs[0], 0.0))
    cs += list(np.random.default_rng(1).uniform(0, 2 * c_ud, 2000))
    for c in cs:
        assert (c < c_ud) == (dist(c) <= ud), c


def _autograd_step(P, u, a, i, j, alpha, lam):
    """cost = log sigmoid(x) - 1/2 lambda sum ||rows||^2 over the gathered rows (FPMC_LR.py:131-143); every gathered row += alpha d cost / d row."""
    import torch
    T = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
    ui = T["ui"][u].clone().requires_grad_(); ai = T["ai"][a].clone().requires_grad_()
    tu = T["iu"][[i, j]].clone().requires_grad_(); ta = T["ia"][[i, j]].clone().requires_grad_()
    x = (tu[0] - tu[1]) @ ui + (ta[0] - ta[1]) @ ai
    los = torch.log(torch.sigmoid(x))
    cost = los - 0.5 * lam * sum((p ** 2).sum() for p in (ui, ai, tu, ta))
    cost.backward()
    out = {k: v.clone() for k, v in T.items()}
    out["ui"][u] += alpha * ui.grad; out["ai"][a] += alpha * ai.grad
    out["iu"][[i, j]] += alpha * tu.grad; out["ia"][[i, j]] += alpha * ta.grad
    return {k: v.numpy() for k, v in out.items()}, float(los.detach())


@pytest.mark.parametrize("case", ["plain", "a_equals_i", "dim64"])
def test_oracle_step_equals_autograd(case):
    rng = np.random.default_rng(7)
    dim = 64 if case == "dim64" else 20
    P = F.init_tables(rng, 5, 30, dim)
    u, a, i, j = 3, 11, 4, 17
    if case == "a_equals_i":
        a = i
    Q, loss = F.step(P, u, a, i, j, 0.01, 0.001)
    R, los = _autograd_step(P, u, a, i, j, 0.01, 0.001)
    assert abs(loss - los) <= 1e-13 * max(1.0, abs(los))
    for k in F.TABLES:
        np.testing.assert_allclose(Q[k], R[k], rtol=0, atol=1e-14)
    moved = {k: np.nonzero(np.any(Q[k] != P[k], axis=1))[0].tolist() for k in F.TABLES}
    assert moved == dict(ui=[u], ai=[a], iu=sorted([i, j]), ia=sorted([i, j]))


def test_batch_rule_of_one_transition_is_the_step_and_counts_rows_per_table():
    rng = np.random.default_rng(3)
    P = F.init_tables(rng, 4, 12, 8)
    Q1, l1 = F.step(P, 1, 2, 3, 5, 0.01, 0.001)
    Qb, lb = F.batch_step(P, np.array([1]), np.array([2]), np.array([3]), np.array([5]), 0.01, 0.001, cap=1.0)
    assert np.isclose(lb[0], l1)
    for k in F.TABLES:
        assert np.array_equal(Q1[k], Qb[k])
    # iu[5] as the positive of one transition and the negative of another: k = 2 -> the mean at cap 1, the sum at cap 2
    u, a, i, j = np.array([0, 1]), np.array([2, 3]), np.array([5, 7]), np.array([6, 5])
    _, d0 = F.transition_terms(P, 0, 2, 5, 6, 0.01, 0.001)
    _, d1 = F.transition_terms(P, 1, 3, 7, 5, 0.01, 0.001)
    want = d0[2][2] + d1[3][2]
    for cap, f in ((1.0, 0.5), (2.0, 1.0), (64.0, 1.0)):
        Qb, _ = F.batch_step(P, u, a, i, j, 0.01, 0.001, cap=cap)
        np.testing.assert_allclose(Qb["iu"][5], P["iu"][5] + f * want, rtol=1e-14)
    # a bad transition (i == j, or an id outside its table) moves nothing and has a NaN loss
    Qb, lb = F.batch_step(P, np.array([0, 9]), np.array([2, 2]), np.array([5, 5]), np.array([5, 6]), 0.01, 0.001)
    assert np.isnan(lb).all() and all(np.array_equal(Qb[k], P[k]) for k in F.TABLES)
