"""POI2Vec fold-in on the host: the rule of tests/foldin_p2v_oracle.py is the xu[u] part of the reference step, its gradient is the
gradient of logsumexp - mean, it descends at the step size the tests use, and the host-side glue (the next-query context rule, the
"history" exclusion lists)."""
import os
import types

import numpy as np
import pytest
import torch

from poi_amd import data as D
from poi_amd.models import _Base
from tests import foldin_p2v_oracle as FO
from tests import poi2vec_oracle as PO
from tests.test_gpu_poi2vec import problem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequences_small.txt")


@pytest.mark.parametrize("alpha", [0.01, 0.1])
@pytest.mark.parametrize("n_item,dim", [(50, 8), (300, 20), (4099, 128)])
def test_one_epoch_is_the_xu_part_of_the_reference_step(n_item, dim, alpha):
    alpha, lam = float(np.float32(alpha)), float(np.float32(0.001))
    pr = problem(200 + dim, n_item, dim, [1, 5, 12])
    for u in range(3):
        t, c = pr["data"][u]
        Q, upq = PO.step(pr["P"], pr["T"], u, t, c, alpha, lam, pr["len_max"])
        F = PO.forward_terms(pr["P"], pr["T"], u, t, c)
        W, loss = FO.fold_in(pr["P"]["wl"], [t], 1, alpha, lam, w0=pr["P"]["xu"][u:u + 1])
        assert np.abs(W[0] - Q["xu"][u]).max() <= 1e-12
        assert abs(loss[0, 0] - (upq + np.log(F["paths"]).mean())) <= 1e-12


def test_gradient_is_autograd_of_logsumexp_minus_mean():
    rng = np.random.default_rng(3)
    wl = rng.uniform(-0.5, 0.5, (257, 20))
    t = np.array([5, 9, 9, 200, 0])
    w = rng.uniform(-0.5, 0.5, 20)
    lam = 0.001
    loss, g = FO.grad(wl, t, w, lam)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    s = torch.tensor(wl) @ wt
    cost = torch.logsumexp(s, 0) - s[torch.tensor(t)].mean()
    (cost + 0.5 * lam * (wt * wt).sum()).backward()
    assert abs(loss - float(cost.detach())) <= 1e-13
    assert np.abs(g - wt.grad.numpy()).max() <= 1e-13


@pytest.mark.parametrize("dim", [8, 64, 128])
def test_losses_fall_strictly_at_alpha_0_1(dim):
    """The objective is convex with curvature at most max_j |wl_j|^2 + lambda; under the reference's uniform(-0.5, 0.5) init that maximum
    stays below 20 at D <= 128 (asserted), so alpha = 0.1 is a descent step: alpha * curvature < 2."""
    rng = np.random.default_rng(dim)
    wl = rng.uniform(-0.5, 0.5, (300, dim)).astype(np.float32).astype(np.float64)
    assert 0.1 * ((wl * wl).sum(axis=1).max() + 0.001) < 2.0
    hist = [rng.integers(0, 300, L) for L in (1, 7, 30)]
    w0 = rng.uniform(-0.5, 0.5, (3, dim))
    _, loss = FO.fold_in(wl, hist, 30, 0.1, 0.001, w0=w0)
    assert np.all(np.diff(loss, axis=1) < 0), loss


def _golden_users():
    rows = [ln.split(" ") for ln in open(GOLDEN).read().strip().split("\n")[1:]]
    return [([int(v) for v in r[3].split("/")], [int(v) for v in r[4].split("/")]) for r in rows]


@pytest.mark.parametrize("thr", [1, 3, 360])
def test_next_context_is_the_loaders_rule(thr):
    for pois, times in _golden_users():
        for gap in (0, 1, thr - 1, thr, 5 * thr):
            now = times[-1] + gap
            brute = [pois[k] for k in range(len(pois) - 1, -1, -1)
                     if all(now - times[m] < thr for m in range(k, len(pois)))]
            got = D.poi2vec_next_context(pois, times, now, thr)
            assert got.tolist() == brute
            if gap < thr:                                    # the query is one more check-in of the loader's sequence
                last = D.poi2vec_contexts(list(times) + [now], thr)[-1]
                assert got.tolist() == [pois[k] for k in last]
    assert D.poi2vec_next_context([], [], 10, 5).tolist() == []
    with pytest.raises(ValueError):
        D.poi2vec_next_context([1, 2], [0], 10, 5)


def test_history_exclusion_lists_are_ascending_and_unique():
    n_item = 40
    hist = [[7, 3, 7, 39, 3], [], [40, 0, 40], [12], [5, 4, 3, 2, 1, 0]]      # (40 = the padding id: no candidate, dropped)
    off = np.zeros(len(hist) + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in hist])
    p = torch.as_tensor(np.concatenate([np.asarray(h, np.int64) for h in hist]).astype(np.int32))
    stub = types.SimpleNamespace(device=torch.device("cpu"), n_item=n_item)
    eo, ex = _Base._foldin_exclusion(stub, "history", torch.as_tensor(off.astype(np.int32)), p, len(hist), int(off[-1]))
    eo, ex = eo.numpy(), ex.numpy()[:int(eo[-1])]
    D.check_exclusion_csr(eo, ex, len(hist), n_item)        # raises unless ascending, unique and in range
    ro, rx = FO.history_exclusion(hist, n_item)
    np.testing.assert_array_equal(eo, ro)
    np.testing.assert_array_equal(ex, rx)


def test_oracle_topk_ex_and_edge_cases():
    s = np.array([[0.1, 0.9, 0.9, 0.3], [0.5, 0.4, 0.3, 0.2]])
    idx, cnt = FO.topk_ex(s, 3, np.array([0, 1, 4]), np.array([1, 0, 1, 3]))
    assert idx.tolist() == [[2, 3, 0], [2, -1, -1]] and cnt.tolist() == [3, 1]
    wl = np.random.default_rng(0).uniform(-0.5, 0.5, (9, 4))
    W, loss = FO.fold_in(wl, [[], [1, 9], [2]], 2, 0.1, 0.0, w0=np.ones((3, 4)))
    assert np.all(W[0] == 1) and np.all(loss[0] == 0) and np.all(np.isnan(W[1])) and np.all(np.isnan(loss[1])) and np.all(np.isfinite(W[2]))
    W0, l0 = FO.fold_in(wl, [[2]], 0, 0.1, 0.0, w0=np.ones((1, 4)))
    assert np.all(W0 == 1) and l0.shape == (1, 0)
