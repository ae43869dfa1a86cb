"""CPU tests of fold-in for the successive-POI models (include/poi_hip.h, poi_foldin_terms_fpmc / poi_foldin_terms_prme / poi_foldin_pair):
the oracle of tests/foldin_seq_oracle.py against the models' own one-transition oracles and against autograd, the exports and their
bindings, and the convergence conditions of tests/test_gpu_foldin_seq.py on the oracle alone."""
import os
import re

import numpy as np

import poi_amd
from tests import foldin_seq_oracle as S
from tests import fpmc_oracle as FO
from tests import prme_oracle as PO
from tests import rank_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, LAM = 0.05, 0.001


def test_one_transition_is_the_ui_row_of_the_fpmc_step():
    rng = np.random.default_rng(1)
    P = {k: S.f32(v) for k, v in FO.init_tables(rng, 5, 30, 12).items()}
    u, a, i, j = 3, 7, 11, 20
    Q, ref_loss = FO.step(P, u, a, i, j, ALPHA, LAM)
    W, L = S.fold_in_fpmc(P, [0, 2], [a, i], [0, j], 0, 1, ALPHA, LAM, w0=P["ui"][u][None])
    al = float(np.float32(ALPHA))
    assert np.abs(W[0] - Q["ui"][u]).max() <= 1e-7 * al          # (the oracle takes alpha / lambda at their float32 values)
    assert abs(L[0, 0] + ref_loss) <= 1e-12
    # p == prev and p == q are legal
    W, L = S.fold_in_fpmc(P, [0, 3], [i, i, 4], [0, 9, 4], 0, 1, ALPHA, LAM, w0=P["ui"][u][None])
    assert np.isfinite(W).all() and np.isfinite(L).all()


def test_one_transition_is_the_du_delta_of_the_prme_step():
    rng = np.random.default_rng(2)
    P = {k: S.f32(v) for k, v in PO.init_tables(rng, 5, 30, 12).items()}
    al, lm, cw = float(np.float32(ALPHA)), float(np.float32(LAM)), float(np.float32(0.2))
    for what, (p, q, prev, d, gap) in dict(near=(11, 20, 7, 2.5, 100), far=(11, 20, 7, 2.5, S.THD + 1), at_thd=(11, 20, 7, 2.5, S.THD),
                                           p_is_prev=(11, 20, 11, 0.0, 100)).items():
        u = 3
        ref_loss, dl = PO.transition_terms(P, u, p, q, prev, d, gap, al, lm, S.THD, cw)
        du = [v for tb, r, v in dl if tb == "du"]
        assert len(du) == 1
        W, L = S.fold_in_prme(P, [0, 2], [prev, p], [0, q], 0, 1, ALPHA, LAM, gap=[0, gap], dist=[0.0, d], thd=S.THD, cw=0.2, w0=P["du"][u][None])
        assert np.abs((W[0] - P["du"][u]) - du[0]).max() <= 1e-13, what
        assert abs(L[0, 0] + ref_loss) <= 1e-12, what          # the reference returns +log sigmoid; fold-in keeps -log sigmoid
    # dist=None: cal_dis of the coordinates
    cordi = np.stack((30.0 + rng.uniform(0, 0.3, 31), 120.0 + rng.uniform(0, 0.3, 31)), axis=1)
    d = float(PO.cal_dis(cordi[11, 0], cordi[11, 1], cordi[7, 0], cordi[7, 1]))
    Wa, La = S.fold_in_prme(P, [0, 2], [7, 11], [0, 20], 0, 1, ALPHA, LAM, gap=[0, 50], cordi=cordi, w0=P["du"][3][None])
    Wb, Lb = S.fold_in_prme(P, [0, 2], [7, 11], [0, 20], 0, 1, ALPHA, LAM, gap=[0, 50], dist=[0.0, d], w0=P["du"][3][None])
    assert np.array_equal(Wa, Wb) and np.array_equal(La, Lb)


def test_oracle_step_is_the_gradient_step_of_the_row():
    """w - alpha d/dw [ -log sigmoid(x) + 0.5 lambda |w|^2 ] in float64 autograd, x of either form."""
    import torch
    rng = np.random.default_rng(5)
    for dim, scale in ((4, 0.5), (20, 2.0), (64, 0.5), (128, 0.1)):
        w, yp, yq = (rng.uniform(-scale, scale, dim) for _ in range(3))
        a, c = float(rng.uniform(0.3, 2.0)), float(rng.uniform(-1, 1))
        for form in (S.DOT, S.METRIC):
            got, loss = S.step(form, w, yp, yq, a, c, ALPHA, LAM)
            tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
            tp, tq = torch.tensor(yp), torch.tensor(yq)
            x = torch.dot(tw, tp - tq) + c if form == S.DOT else a * (((tw - tq) ** 2).sum() - ((tw - tp) ** 2).sum()) + c
            cost = -torch.nn.functional.logsigmoid(x) + 0.5 * LAM * (tw ** 2).sum()
            cost.backward()
            want = w - ALPHA * tw.grad.numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (dim, form)
            assert abs(loss - float(-torch.nn.functional.logsigmoid(x).detach())) <= 1e-12 * max(1.0, loss)


def test_oracle_edges_skips_and_bad_users():
    P = S.toy(3, 8, [0, 1, 4, 3], 2)
    T = dict(iu=P["y"], ia=P["s"], ai=P["v"])
    W, L = S.fold_in_fpmc(T, P["off"], P["p"], P["q"], P["total"], 0, ALPHA, LAM, P["w0"])
    assert np.array_equal(W, P["w0"]) and L.shape == (4, 0)
    W, L = S.fold_in_fpmc(T, P["off"], P["p"], P["q"], P["total"], 2, ALPHA, LAM)
    assert not W[:2].any() and not L[:2].any() and (L[2:] > 0).all()          # lengths 0 and 1: no transition
    # a -1 negative skips its step: the same as the history with that step's update removed
    q = P["q"].copy(); t = int(P["off"][2]) + 2
    q[t] = -1; q[P["total"] + t] = -1
    Ws, Ls = S.fold_in_fpmc(T, P["off"], P["p"], q, P["total"], 2, ALPHA, LAM)
    tm = S.terms("fpmc", T, P["off"], P["p"], P["q"], P["total"], 2)
    w, loss = np.zeros(8), np.zeros(2)
    for e in range(2):
        for s in range(int(P["off"][2]) + 1, int(P["off"][3])):
            if s == t:
                continue
            w, l = S.step(S.DOT, w, T["iu"][P["p"][s]], T["iu"][P["q"][e * P["total"] + s]], 1.0, tm["c"][e, s], float(np.float32(ALPHA)), float(np.float32(LAM)))
            loss[e] += l
    assert np.array_equal(Ws[2], w) and np.array_equal(Ls[2], loss) and np.array_equal(Ws[3], W[3])
    # an id outside the table, a bad distance: that user alone is NaN
    bad = P["p"].copy(); bad[int(P["off"][3])] = P["n_item"] + 1           # the first check-in of user 3: only ever a prev
    Wb, Lb = S.fold_in_fpmc(T, P["off"], bad, P["q"], P["total"], 2, ALPHA, LAM)
    assert np.isnan(Wb[3]).all() and np.isnan(Lb[3]).all() and np.array_equal(Wb[:3], W[:3]) and np.array_equal(Lb[:3], L[:3])
    Tp = dict(dp=P["y"], ds=P["s"])
    Wp, Lp = S.fold_in_prme(Tp, P["off"], P["p"], P["q"], P["total"], 2, ALPHA, LAM, P["gap"], P["dist"], thd=S.THD)
    for v in (-1.0, np.inf, np.nan):
        d = P["dist"].copy(); d[int(P["off"][2]) + 1] = v
        Wd, Ld = S.fold_in_prme(Tp, P["off"], P["p"], P["q"], P["total"], 2, ALPHA, LAM, P["gap"], d, thd=S.THD)
        assert np.isnan(Wd[2]).all() and np.isnan(Ld[2]).all() and np.array_equal(Wd[3], Wp[3]) and np.array_equal(Ld[3], Lp[3])


def test_dot_form_without_terms_is_the_bpr_fold_in():
    from tests import foldin_oracle as F
    P = S.toy(4, 12, [0, 1, 5, 7], 2)
    W, L = S.chain(S.DOT, P["y"], P["off"], P["p"], P["q"], P["total"], 2, ALPHA, LAM, w0=P["w0"], first=0)
    Wb, Lb = F.fold_in(P["y"], P["off"], P["p"], P["q"], P["total"], 2, ALPHA, LAM, P["w0"])
    assert np.array_equal(W, Wb) and np.array_equal(L, Lb)


def _header_params(code, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
    assert m, "include/poi_hip.h does not declare %s" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_declares_the_entries_the_binding_takes():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("poi_foldin_terms_fpmc", 11), ("poi_foldin_terms_prme", 17), ("poi_foldin_pair", 21)):
        assert len(_header_params(code, name)) == len(poi_amd._lib.SIGNATURES[name][1]) == n_args, name
    assert '"foldin_terms"' in hdr and '"foldin_pair"' in hdr
    assert re.search(r"POI_FOLDIN_DOT\s*=\s*0\s*,\s*POI_FOLDIN_METRIC\s*=\s*1", code)
    assert (poi_amd._lib.FOLDIN_DOT, poi_amd._lib.FOLDIN_METRIC) == (0, 1)


def test_library_exports_the_entries():
    poi_amd.build.build_lib()
    lib = poi_amd._lib.load()
    assert all(hasattr(lib, n) for n in ("poi_foldin_terms_fpmc", "poi_foldin_terms_prme", "poi_foldin_pair")) and lib.poi_abi_version() == 9


def test_models_offer_the_methods():
    from poi_amd import models
    for cls in (models.OboFpmc_lr, models.OboPrme, models.OboPRPRM):
        assert all(callable(getattr(cls, m, None)) for m in ("fold_in", "recommend_new", "rank_new")), cls


def learn_scores(model, P, W):
    """The model's score rows for the folded rows W (query / last POI = the history's last check-in)."""
    c = S.LEARN
    last = P["hist"][:, -1]
    if model == "fpmc":
        return W @ P["y"][:c["n_item"]].T + P["v"][last] @ P["s"][:c["n_item"]].T
    return PO.score_rows(dict(du=W, dp=P["y"], ds=P["s"]), P["cordi"], np.arange(c["n"]), last, cw=float(np.float32(c["cw"])))


def learn_oracle(model, P):
    c = S.LEARN
    if model == "fpmc":
        return S.fold_in_fpmc(dict(iu=P["y"], ia=P["s"], ai=P["v"]), P["off"], P["p"], P["q"], 0, c["epochs"], c["alpha"], c["lam"], P["w0"])
    return S.fold_in_prme(dict(dp=P["y"], ds=P["s"]), P["off"], P["p"], P["q"], 0, c["epochs"], c["alpha"], c["lam"], P["gap"], P["dist"],
                          thd=S.THD, cw=c["cw"], w0=P["w0"])


def test_the_oracle_learns_on_the_gpu_tests_inputs():
    """The two conditions of test_gpu_foldin_seq.py::test_it_learns hold for the rules themselves on those exact inputs."""
    P = S.learn_problem()
    tgt = P["hist"][:, 1:]
    ones = np.ones_like(tgt)
    for model in ("fpmc", "prme"):
        W, L = learn_oracle(model, P)
        assert L[:, -1].mean() < L[:, 0].mean(), model
        before = RO.ranks(learn_scores(model, P, P["w0"]), tgt, ones)["rank"]
        after = RO.ranks(learn_scores(model, P, W), tgt, ones)["rank"]
        print("%s: epoch losses %s, mean rank %.1f -> %.1f" % (model, np.round(L.sum(0), 2), before.mean(), after.mean()))
        assert after.mean() < 0.9 * before.mean(), "%s: the inputs must leave a clear margin" % model
