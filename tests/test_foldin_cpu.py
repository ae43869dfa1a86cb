"""CPU tests of the fold-in rule (include/poi_hip.h, poi_foldin_bpr): the oracle of tests/foldin_oracle.py against autograd, the export
and its binding, and the convergence condition of tests/test_gpu_foldin.py on the oracle alone."""
import os
import re

import numpy as np

import poi_amd
from tests import foldin_oracle as F
from tests import rank_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_step_is_the_user_row_gradient_step():
    """w - alpha d/dw [ -log sigmoid(w . d) + 0.5 lambda |w|^2 ] (public/BPR.py:216-230: the usr part of the cost) in float64 autograd."""
    import torch
    rng = np.random.default_rng(5)
    for dim, scale in ((8, 0.5), (20, 3.0), (64, 0.5), (256, 0.05)):
        w, yp, yq = (rng.uniform(-scale, scale, dim) for _ in range(3))
        alpha, lam = 0.05, 0.001
        got, loss = F.step(w, yp, yq, alpha, lam)
        tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        x = torch.dot(tw, torch.tensor(yp - yq))
        cost = -torch.nn.functional.logsigmoid(x) + 0.5 * lam * (tw ** 2).sum()
        cost.backward()
        want = w - alpha * tw.grad.numpy()
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        assert abs(loss - float(-torch.nn.functional.logsigmoid(x).detach())) <= 1e-13 * max(1.0, loss)
    # p == q: only the decay acts
    got, loss = F.step(w, yp, yp, alpha, lam)
    assert np.allclose(got, w * (1 - alpha * lam), rtol=0, atol=1e-15) and abs(loss - np.log(2.0)) < 1e-15


def test_oracle_edges():
    P = F.toy(3, 8, [0, 3, 2], 2)
    W, L = F.fold_in(P["items"], P["off"], P["p"], P["q"], P["total"], 0, 0.05, 0.001, P["w0"])
    assert np.array_equal(W, P["w0"]) and L.shape == (3, 0)
    W, L = F.fold_in(P["items"], P["off"], P["p"], P["q"], P["total"], 2, 0.05, 0.001)
    assert np.array_equal(W[0], np.zeros(8)) and np.array_equal(L[0], [0.0, 0.0]) and (L[1:] > 0).all()
    bad = P["p"].copy(); bad[4] = P["n_item"] + 1
    Wb, Lb = F.fold_in(P["items"], P["off"], bad, P["q"], P["total"], 2, 0.05, 0.001)
    assert np.isnan(Wb[2]).all() and np.isnan(Lb[2]).all() and np.array_equal(Wb[:2], W[:2]) and np.array_equal(Lb[:2], L[:2])


def test_header_declares_the_entry_the_binding_takes():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+poi_foldin_bpr\s*\(([^)]*)\)", code)
    assert m, "include/poi_hip.h does not declare poi_foldin_bpr"
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert len(params) == len(poi_amd._lib.SIGNATURES["poi_foldin_bpr"][1]) == 16
    assert '"foldin"' in hdr


def test_library_exports_the_entry():
    poi_amd.build.build_lib()
    lib = poi_amd._lib.load()
    assert hasattr(lib, "poi_foldin_bpr") and lib.poi_abi_version() == 9


def test_the_oracle_learns_on_the_gpu_tests_inputs():
    """The two conditions of test_gpu_foldin.py::test_it_learns hold for the rule itself on those exact inputs."""
    c, P = F.LEARN, F.learn_problem()
    W, L = F.fold_in(P["items"], P["off"], P["p"], P["q"], 0, c["epochs"], c["alpha"], c["lam"], P["w0"])
    assert L[:, -1].sum() < L[:, 0].sum()
    Y = P["items"][:c["n_item"]]
    ones = np.ones_like(P["hist"])
    before = RO.ranks(P["w0"] @ Y.T, P["hist"], ones)["rank"]
    after = RO.ranks(W @ Y.T, P["hist"], ones)["rank"]
    print("epoch losses %s, mean rank %.1f -> %.1f" % (np.round(L.sum(0), 2), before.mean(), after.mean()))
    assert after.mean() < 0.8 * before.mean(), "the inputs must leave a clear margin"
