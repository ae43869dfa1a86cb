"""Fixture conditions of tests/reject_cases.py, no GPU: the reserved rows are named by no kept element, the window-edge cases fill whole
64-touch windows, and the BPR fixtures are ones on which the clamped-key rule of the old csrc/bpr.hip (a rejected triple's touches stay in
the runs of the rows its ids clamp to: +1 multiplicity, an L2 decay) misses the suite's per-row update bar - so that the GPU half
(tests/test_gpu_rejected.py) cannot pass vacuously.  These are conditions on the inputs, not tolerances on a kernel."""
import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import reject_cases as RC
from tests.gpu_util import delta_excess, round_f32
from tests.test_gpu_bpr import _expected_vec

STEPS = tuple(RC.SPECS)
ALL = {s: RC.build(s) for s in STEPS}
DISJOINT = RC.build("bpr", disjoint=True)


@pytest.mark.parametrize("step", STEPS)
def test_every_placement_is_there_and_reserved_rows_are_named_by_no_kept_element(step):
    cases = ALL[step]
    want = ["first", "last", "edge-1", "edge", "edge+1", "long_run", "all_rejected", "n1", "sole", "all_bad"] + ["kind:" + k for k in RC.SPECS[step].kinds]
    assert list(cases) == want
    for c in list(cases.values()) + (list(DISJOINT.values()) if step == "bpr" else []):
        n = len(c.launch[RC.SPECS[step].user])
        assert n <= 300 and len(c.keep) + len(c.rejected) == n and len(c.rejected) >= 1
        users, pois = RC.named_rows(step, c.launch, c.keep)
        assert not np.intersect1d(users, c.res_user).size and not np.intersect1d(pois, c.res_poi).size, c.name
        assert users.size == 0 or (users.min() >= 0 and users.max() < RC.N_USER and pois.min() >= 0 and pois.max() <= RC.N_ITEM)
    assert cases["first"].rejected.tolist() == [0] and cases["last"].rejected.tolist() == [len(cases["last"].keep)]
    assert len(cases["all_rejected"].keep) == 0 and len(cases["n1"].rejected) == 1 and len(cases["n1"].keep) == 0
    r = cases["long_run"].rejected
    assert len(r) == RC.LONG and np.array_equal(r, np.arange(r[0], r[0] + RC.LONG))       # consecutive; >= 70 touches in every part
    # sole: the valid ids of its rejected elements name reserved rows only; all_bad: no valid id at all
    s = RC.SPECS[step]
    c = cases["sole"]
    assert len(c.rejected) == len(s.kinds)
    for t in c.rejected:
        u = c.launch[s.user][t]
        assert not 0 <= u < RC.N_USER or u in c.res_user
        assert all(not 0 <= c.launch[f][t] <= RC.N_ITEM or c.launch[f][t] in c.res_poi for f in s.poi)
    c = cases["all_bad"]
    t = int(c.rejected[0])
    ids = [int(c.launch[f][t]) for f in (s.user,) + s.poi]
    assert not 0 <= ids[0] < RC.N_USER and all(not 0 <= v <= RC.N_ITEM for v in ids[1:])
    assert min(ids) < 0 and (1 << 20) in ids


def test_disjoint_bpr_cases_share_no_row():
    for c in DISJOINT.values():
        u = c.launch["u"][c.keep]
        pq = np.concatenate([c.launch["p"][c.keep], c.launch["q"][c.keep]])
        assert len(np.unique(u)) == len(u) and len(np.unique(pq)) == len(pq), c.name


@pytest.mark.parametrize("step", STEPS)
def test_window_edge_cases_fill_whole_windows(step):
    """valid touches per sorted part, from the keys: WINDOW kept elements give a multiple of 64 (the sentinel run starts on a window
    start), one fewer / one more do not; the sentinel run of long_run is longer than a window in every part"""
    cases = ALL[step]
    for d, name in ((-1, "edge-1"), (0, "edge"), (1, "edge+1")):
        parts = RC.part_keys(step, cases[name].launch)
        kept = len(cases[name].keep)
        assert kept == RC.WINDOW[step] + d
        for part, keys in zip(RC.SPECS[step].parts, parts):
            valid = int((keys >= 0).sum())
            assert valid == kept * len(part), (name, valid)          # every kept element has all its touches
            assert (valid % 64 == 0) == (d == 0), (name, valid)
            assert len(keys) - valid == 3 * len(part)
    for keys in RC.part_keys(step, cases["long_run"].launch):
        assert (keys < 0).sum() > 64


# ---- BPR: the clamped-key rule misses the bar on these fixtures ------------------------------------------------------------------
def _clamped_model(P, u, p, q, keep, alpha, lam, cap):
    """The rule the old bpr_keys / bpr_chunk applied: the kept triples' gradient sums, but every row a rejected triple's CLAMPED ids name
    (min((unsigned) id, last row): a bad user -> n_user - 1, a bad POI -> the pad row) counts its touches in k:
    row -= alpha min(k, cap) (sum / k + lambda row).  Gradient sums from _expected_vec at alpha 1, lambda 0, no cap: T - new = G."""
    uk, pk, qk = u[keep], p[keep], q[keep]
    flat, _ = _expected_vec(P, uk, pk, qk, 1.0, 0.0, 1e30)
    out = {}
    for name, ids, last in (("ux", [u], RC.N_USER - 1), ("lt", [p, q], RC.N_ITEM)):
        T = np.asarray(P[name], np.float64)
        G = T - flat[name]
        k = np.zeros(T.shape[0])
        for a in ids:
            np.add.at(k, np.where((a < 0) | (a > last), last, a), 1)
        sc = np.where(k > 0, alpha * np.minimum(k, cap), 0.0)
        out[name] = T - sc[:, None] * (G / np.maximum(k, 1)[:, None] + lam * T)
    return out


@pytest.fixture(scope="module")
def bpr_P():
    return {d: round_f32(O.init_bpr_params(np.random.default_rng(70 + d), RC.N_USER, RC.N_ITEM, d)) for d in (20, 64)}


def test_clamped_model_is_the_batch_rule_on_a_clean_launch(bpr_P):
    c = ALL["bpr"]["first"]
    u, p, q = (c.launch[f][c.keep] for f in "upq")
    for cap in (1.0, 8.0, 1e9):
        a = _clamped_model(bpr_P[64], u, p, q, np.arange(len(u)), 0.01, 0.001, cap)
        b, _ = _expected_vec(bpr_P[64], u, p, q, 0.01, 0.001, cap)
        assert np.allclose(a["ux"], b["ux"], rtol=1e-13, atol=1e-15) and np.allclose(a["lt"], b["lt"], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("dim", [20, 64])
def test_bpr_fixtures_separate_the_clamped_rule_from_the_contract(bpr_P, dim):
    P = bpr_P[dim]
    for name, c in ALL["bpr"].items():
        if not len(c.keep):
            continue
        u, p, q = (c.launch[f] for f in "upq")
        for cap in (1.0, 8.0, 1e9):
            exp, _ = _expected_vec(P, u[c.keep], p[c.keep], q[c.keep], 0.01, 0.001, cap)
            got = _clamped_model(P, u, p, q, c.keep, 0.01, 0.001, cap)
            ex = max(delta_excess(got[k], exp[k], P[k])[0] for k in ("ux", "lt"))
            print("bpr clamped-key model, dim %d %-8s cap %-5g: delta_excess %.1f" % (dim, name, cap, ex))
            if name.startswith("kind:") and cap <= 8.0:
                assert ex >= 10.0, (name, cap, ex)
            if name == "sole" and cap == 1e9:      # the decay alone: the reserved rows change bits in float32
                f32 = lambda a: np.asarray(a, np.float32)
                assert not np.array_equal(f32(got["ux"])[c.res_user], f32(P["ux"])[c.res_user])
                assert not np.array_equal(f32(got["lt"])[c.res_poi], f32(P["lt"])[c.res_poi])
                assert np.array_equal(f32(exp["ux"])[c.res_user], f32(P["ux"])[c.res_user])
                assert np.array_equal(f32(exp["lt"])[c.res_poi], f32(P["lt"])[c.res_poi])


def test_user_cases_cover_the_placements():
    good, bad = list(range(12)), {"target": 12, "user_high": 40, "user_neg": -1}
    cases = RC.user_cases(good, bad)
    assert list(cases) == ["first", "last", "long_run", "all_rejected", "n1", "kind:target", "kind:user_high", "kind:user_neg"]
    for c in cases.values():
        assert sorted(c.users[c.keep].tolist()) == good or not len(c.keep)
        assert set(c.users[c.rejected].tolist()) <= set(bad.values()) and len(c.rejected) >= 1
    assert len(cases["long_run"].rejected) == RC.LONG and len(cases["all_rejected"].keep) == 0 and len(cases["n1"].users) == 1
