"""CPU: the sparse CA-RNN batch oracle (oracle/poi_oracle.py carnn_batch_step, what tests/test_gpu_carnn_launch_sizes.py holds the device
to at launches of thousands of sequences) against the construction the toy-size tests use - carnn_step per sequence, one dense
parameter set each, combined by tests/gpu_util.batch_mean_update: all three tensors to 1e-12 relative (weights and updates), the losses,
and the touched sets, with sequences of one and two positions, repeated POIs inside a sequence and POIs that are a positive of one
sequence and a negative of another; from the padded tables and from CSR tables; the same bits whatever the number of threads."""
import types

import numpy as np
import pytest

from oracle import poi_oracle as O
from tests.gpu_util import batch_mean_update, rel_err, round_f32, toy_problem

ALPHA, LAMBDA = 0.01, 0.001
NAMES = ("lt", "wd", "M")


def _dense_construction(P, T, users):
    """tests/test_gpu_carnn.py test_carnn_batch_matches_the_batch_rule, verbatim."""
    Pm, Qm, DPm, DQm, Mm = T["train"][0], T["train"][2], T["dist"][0], T["dist"][2], T["train"][1]
    news, touched, losses = [], [], []
    for u in users:
        Pn, los = O.carnn_step(P, Pm[u], Qm[u], DPm[u], DQm[u], Mm[u], ALPHA, LAMBDA)
        news.append(Pn); losses.append(los)
        touched.append(dict(lt=np.unique(np.concatenate((Pm[u], Qm[u]))), wd=np.unique(np.concatenate((DPm[u], DQm[u])))))
    exp = batch_mean_update(P, news, touched, ("lt",), ("M",))
    acc = np.zeros_like(P["wd"]); cnt = np.zeros(P["wd"].shape[0])
    for Pn, tch in zip(news, touched):
        acc[tch["wd"]] += Pn["wd"][tch["wd"]] - P["wd"][tch["wd"]]; cnt[tch["wd"]] += 1
    exp["wd"] = P["wd"] + acc / np.maximum(cnt, 1)[:, None, None]
    t_lt = np.zeros(P["lt"].shape[0], bool); t_wd = np.zeros(P["wd"].shape[0], bool)
    for tch in touched:
        t_lt[tch["lt"]] = True; t_wd[tch["wd"]] = True
    return exp, np.asarray(losses), t_lt, t_wd


def _padded(T):
    return (T["train"][0], T["train"][2], T["dist"][0], T["dist"][2], T["train"][1])


def _check(P, T, users, what, threads=1):
    exp, losses, t_lt, t_wd = _dense_construction(P, T, users)
    got, glos, g_lt, g_wd = O.carnn_batch_step(P, _padded(T), users, ALPHA, LAMBDA, threads=threads)
    assert np.array_equal(g_lt, t_lt) and np.array_equal(g_wd, t_wd), what
    assert glos.shape == losses.shape and rel_err(glos, losses) <= 1e-12, (what, rel_err(glos, losses))
    for k in NAMES:
        assert got[k].shape == exp[k].shape
        assert rel_err(got[k], exp[k]) <= 1e-12, (what, k, rel_err(got[k], exp[k]))
        assert rel_err(got[k] - P[k], exp[k] - P[k]) <= 1e-12, (what, k, "update", rel_err(got[k] - P[k], exp[k] - P[k]))
    assert np.array_equal(got["lt"][~t_lt], P["lt"][~t_lt]) and np.array_equal(got["wd"][~t_wd], P["wd"][~t_wd])
    return got, glos


def _edges(T, users):
    """(has a sequence of one position, of two, a POI repeated inside a sequence, a POI that is p of one sequence and q of another)"""
    Pm, Qm, lens = T["train"][0], T["train"][2], T["lens"]
    rep = any(len(np.unique(Pm[u][:lens[u]])) < lens[u] for u in users)
    ps = {int(x): int(u) for u in users for x in Pm[u][:lens[u]]}
    cross = any(int(x) in ps and ps[int(x)] != int(u) for u in users for x in Qm[u][:lens[u]])
    return bool((lens[users] == 1).any()), bool((lens[users] == 2).any()), rep, cross


@pytest.mark.parametrize("dim,n_dist,min_len", [(32, 11, 4), (64, 11, 4), (128, 200, 4), (64, 700, 4), (64, 11, 1), (128, 37, 1)])
def test_sparse_batch_oracle_on_the_toy_shapes_of_the_gpu_test(dim, n_dist, min_len):
    T = toy_problem(520, n_user=40, n_item=90, n_dist=n_dist, dim=dim, len_max=10, hot=25, min_len=min_len)
    P = round_f32(O.init_carnn_params(np.random.default_rng(520 + 3000), T["n_item"], T["n_dist"], T["dim"]))
    users = np.random.default_rng(1).permutation(40)[:37].astype(np.int32)
    one, two, rep, cross = _edges(T, users)
    assert rep and cross and (min_len > 1 or (one and two))
    _check(P, T, users, "toy dim %d, %d bins, min_len %d" % (dim, n_dist, min_len), threads=3)


def test_sparse_batch_oracle_on_random_configurations():
    """20 draws in the style of tools/fuzz_carnn.py (its dims and tables small enough for a dense parameter set per sequence)."""
    seen = np.zeros(4, int)
    for s in range(20):
        rng = np.random.default_rng(47_000 + s)
        dim = int(rng.choice([20, 32, 64, 128]))
        n_dist = int(rng.choice([3, 11, 40, 200]))
        n_item = int(rng.choice([17, 64, 129, 400]))
        n_user = int(rng.integers(1, 25))
        len_max = int(rng.integers(2, 13))
        min_len = int(rng.integers(1, len_max + 1)) if s % 2 else 1
        T = toy_problem(9500 + s, n_user=n_user, n_item=n_item, n_dist=n_dist, dim=dim, len_max=len_max, min_len=min_len, hot=max(2, n_item // 3))
        P = round_f32(O.init_carnn_params(np.random.default_rng(s + 3000), n_item, n_dist, dim))
        k = int(rng.integers(1, n_user + 1))
        users = rng.permutation(n_user)[:k].astype(np.int32)
        seen += _edges(T, users)
        _check(P, T, users, "config %d: dim %d, %d bins, %d POIs, %d of %d users, L <= %d" % (s, dim, n_dist, n_item, k, n_user, len_max),
               threads=1 + s % 4)
    assert (seen >= 3).all(), seen          # every edge case in several draws


def test_sparse_batch_oracle_one_sequence_is_the_reference_step():
    T = toy_problem(77, n_user=6, n_item=50, n_dist=11, dim=20, len_max=9, min_len=1)
    P = round_f32(O.init_carnn_params(np.random.default_rng(5), 50, 11, 20))
    for u in range(6):
        Pn, los = O.carnn_step(P, T["train"][0][u], T["train"][2][u], T["dist"][0][u], T["dist"][2][u], T["train"][1][u], ALPHA, LAMBDA)
        got, glos, _, _ = O.carnn_batch_step(P, _padded(T), [u], ALPHA, LAMBDA)
        assert glos[0] == los
        assert all(rel_err(got[k], Pn[k]) <= 1e-15 for k in NAMES)


def test_sparse_batch_oracle_is_deterministic_and_reads_csr_tables():
    """Same bits from 1, 2 and 16 threads and from any block size (the sums run in sequence order), and from CSR tables padded with
    (n_item, n_dist) as from the padded tables."""
    T = toy_problem(91, n_user=50, n_item=120, n_dist=37, dim=32, len_max=12, min_len=1, hot=30)
    P = round_f32(O.init_carnn_params(np.random.default_rng(6), 120, 37, 32))
    users = np.random.default_rng(2).permutation(50)[:45]
    ref = O.carnn_batch_step(P, _padded(T), users, ALPHA, LAMBDA, threads=1)
    lens = T["lens"]
    off = np.concatenate(([0], np.cumsum(lens)))
    flat = lambda m: np.concatenate([m[u][:lens[u]] for u in range(50)])
    csr = types.SimpleNamespace(off=off, p=flat(T["train"][0]), q=flat(T["train"][2]), dp=flat(T["dist"][0]), dq=flat(T["dist"][2]), len_max=12)
    for tables, threads, block in ((_padded(T), 2, 32), (_padded(T), 16, 5), (csr, 4, 32)):
        got = O.carnn_batch_step(P, tables, users, ALPHA, LAMBDA, threads=threads, block=block)
        assert all(np.array_equal(got[0][k], ref[0][k]) for k in NAMES)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:]))


def test_per_sequence_helper_runs_in_float32():
    """The shared helper computes in the dtype of its tables: float32 tables give float32 gradients close to the float64 ones (what the
    launch-size test would use to tell rounding of a long sequence from a kernel bug)."""
    T = toy_problem(33, n_user=3, n_item=40, n_dist=11, dim=32, len_max=12, min_len=12)
    P = round_f32(O.init_carnn_params(np.random.default_rng(7), 40, 11, 32))
    P32 = {k: v.astype(np.float32) for k, v in P.items()}
    a = (T["train"][0][0], T["train"][2][0], T["dist"][0][0], T["dist"][2][0], T["train"][1][0], LAMBDA)
    r64, r32 = O._carnn_seq_grads(P, *a), O._carnn_seq_grads(P32, *a)
    assert r32[1].dtype == np.float32 and r32[3].dtype == np.float32 and r32[4].dtype == np.float32
    assert all(rel_err(r32[i], r64[i]) < 1e-4 for i in (1, 3, 4)) and abs(r32[5] - r64[5]) < 1e-4 * abs(r64[5])
