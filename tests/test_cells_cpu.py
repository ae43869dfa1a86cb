"""CPU checks of tests/cells_oracle.py (the oracle of the -m gpu Lstm / Rnn tests): against torch-autograd of a literal transcription
of the reference's Theano graph (public/GRU.py:525-605 Lstm, :682-760 Rnn), the padding rule, and a hand-worked Lstm."""
import math

import numpy as np
import pytest
import torch

from tests import cells_oracle as C

ALPHA, LAM = 0.01, 0.001


def _batch(seed, n, n_item, len_max, lens, hot=6):
    rng = np.random.default_rng(seed)
    P = np.full((n, len_max), n_item); Q = P.copy(); M = np.zeros((n, len_max), int)
    for u, L in enumerate(lens):
        P[u, :L] = rng.integers(0, hot, L)                    # few distinct POIs: duplicates within and across users
        Q[u, :L] = rng.integers(hot // 2, n_item, L)
        M[u, :L] = 1
    return P, Q, M


def _params(seed, n_item, dim, cell):
    rng = np.random.default_rng(seed)
    P = C.init_params(rng, n_item, dim, cell)
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape)
    return P


def reference_step(P, pidxs, qidxs, tra_mask, alpha, lam, cell):
    """The reference graph, line by line, in torch float64: a masked batched scan to the batch's longest length with the pad rows
    fed to the cell, bi allocated per user, the cost of :582-588 / :737-743, dense updates and the Unique write-back of lt."""
    T = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.items()}
    lt, ui, wh = T["lt"], T["ui"], T["wh"]
    pid, qid, mask = torch.as_tensor(pidxs), torch.as_tensor(qidxs), torch.as_tensor(tra_mask)
    n, D = mask.shape[0], lt.shape[1]
    seq_length = int(mask.sum(1).max())
    xps, xqs = lt[pid].permute(1, 0, 2), lt[qid].permute(1, 0, 2)                  # (len_max, n, D)
    h = torch.zeros(n, D, dtype=torch.float64)
    c = torch.zeros(n, D, dtype=torch.float64)
    losses = []
    if cell == "lstm":
        bi = T["bi"].expand(n, 4, D).permute(1, 2, 0)                              # (4, D, n)
    else:
        bi = T["bi"].expand(n, D).T                                                # (D, n)
    for t in range(seq_length):
        xp_t, xq_t, mask_t = xps[t], xqs[t], mask[:, t].to(torch.float64)
        upq_t = (h * (xp_t - xq_t)).sum(1)
        if cell == "lstm":
            gates = torch.matmul(ui, xp_t.T) + torch.matmul(wh, h.T) + bi          # (4, D, n)
            i, f, g, o = torch.sigmoid(gates[0]).T, torch.sigmoid(gates[1]).T, torch.tanh(gates[2]).T, torch.sigmoid(gates[3]).T
            c = f * c + i * g
            h = o * torch.tanh(c)
        else:
            h = torch.sigmoid(torch.matmul(ui, xp_t.T) + torch.matmul(wh, h.T) + bi).T
        losses.append(torch.log(torch.sigmoid(upq_t)) * mask_t)
    upq = torch.stack(losses).sum()
    seq_l2_sq = sum((par ** 2).sum() for par in (xps, xqs, ui, wh)) + (bi ** 2).sum() / n
    cost = -upq / n + 0.5 * lam * seq_l2_sq
    grads = torch.autograd.grad(cost, [T[k] for k in ("lt", "ui", "wh", "bi")])
    N = {k: np.asarray(P[k], np.float64).copy() for k in P}
    for k, g in zip(("ui", "wh", "bi"), grads[1:]):
        N[k] = N[k] - alpha * g.numpy()
    uiq = np.unique(np.concatenate((np.asarray(pidxs), np.asarray(qidxs))))
    N["lt"][uiq] = N["lt"][uiq] - alpha * grads[0].numpy()[uiq]
    return N, float(-upq.detach())


CASES = [("ragged", 5, [7, 3, 5, 2, 6], 9), ("full_and_short", 4, [8, 1, 2, 8], 8), ("one_user", 1, [6], 9), ("one_user_len1", 1, [1], 4),
         ("duplicates", 6, [4, 4, 4, 4, 4, 4], 5)]


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("name,n,lens,len_max", CASES, ids=[c[0] for c in CASES])
def test_oracle_matches_autograd_of_the_reference_graph(cell, name, n, lens, len_max):
    n_item, dim = 17, 6
    P = _params(11, n_item, dim, cell)
    pm, qm, mm = _batch(3, n, n_item, len_max, lens, hot=3 if name == "duplicates" else 6)
    for step in range(2):                                                          # the second step starts from moved tables
        ref, ref_loss = reference_step(P, pm, qm, mm, ALPHA, LAM, cell)
        got, loss = C.minibatch_step(P, pm, qm, mm, ALPHA, LAM, cell)
        assert abs(loss - ref_loss) <= 1e-10 * max(1.0, abs(ref_loss)), (loss, ref_loss)
        for k in ("lt", "ui", "wh", "bi"):
            assert got[k].shape == ref[k].shape
            assert np.max(np.abs(got[k] - ref[k])) <= 1e-10, (k, step, np.max(np.abs(got[k] - ref[k])))
        P = got


@pytest.mark.parametrize("cell", C.CELLS)
def test_dead_steps_are_exact(cell):
    """A 2-position user next to a 9-position one: the reference graph feeds the short user seven pad rows; the per-sequence oracle
    runs its single cell step and stops.  Both give the same tables to 1e-10: the dead steps are exactly dead."""
    n_item, dim = 12, 4
    P = _params(5, n_item, dim, cell)
    pm, qm, mm = _batch(8, 2, n_item, 9, [9, 2])
    ref, _ = reference_step(P, pm, qm, mm, ALPHA, LAM, cell)
    got, _ = C.minibatch_step(P, pm, qm, mm, ALPHA, LAM, cell)
    assert np.max(np.abs(got["lt"] - ref["lt"])) <= 1e-10


@pytest.mark.parametrize("cell", C.CELLS)
def test_len_max_changes_only_the_pad_row(cell):
    n_item, dim, n = 15, 4, 3
    P = _params(2, n_item, dim, cell)
    pm, qm, mm = _batch(4, n, n_item, 7, [7, 3, 5])
    a, la = C.minibatch_step(P, pm, qm, mm, ALPHA, LAM, cell)
    extra = 3
    pad = lambda t, v: np.concatenate((t, np.full((n, extra), v)), axis=1)
    b, lb = C.minibatch_step(P, pad(pm, n_item), pad(qm, n_item), pad(mm, 0), ALPHA, LAM, cell)
    assert la == lb
    for k in ("ui", "wh", "bi"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["lt"][:n_item], b["lt"][:n_item])
    d_mult = 2 * extra * n
    assert np.allclose(a["lt"][n_item] - b["lt"][n_item], ALPHA * LAM * d_mult * P["lt"][n_item], rtol=1e-12, atol=0)
    ref, _ = reference_step(P, pad(pm, n_item), pad(qm, n_item), pad(mm, 0), ALPHA, LAM, cell)
    assert np.max(np.abs(b["lt"] - ref["lt"])) <= 1e-10


def test_hand_worked_two_step_lstm():
    """D = 1, one user, three positions = two cell steps, every quantity written out as a scalar."""
    sg = lambda x: 1.0 / (1.0 + math.exp(-x))
    lt = np.array([[0.3], [-0.2], [0.5], [0.1], [0.4]])       # POIs 0 .. 3, pad row 4
    ui = np.array([0.2, -0.3, 0.4, 0.1]).reshape(4, 1, 1); wh = np.array([-0.1, 0.25, 0.35, -0.45]).reshape(4, 1, 1)
    bi = np.array([0.05, -0.05, 0.1, 0.0]).reshape(4, 1)
    p, q = [0, 2, 1], [3, 1, 0]
    x = [lt[i, 0] for i in p]; e = [lt[i, 0] - lt[j, 0] for i, j in zip(p, q)]
    U, W, B = ui.ravel(), wh.ravel(), bi.ravel()

    def step(xt, h, c):
        a = [U[k] * xt + W[k] * h + B[k] for k in range(4)]
        i, f, g, o = sg(a[0]), sg(a[1]), math.tanh(a[2]), sg(a[3])
        cn = f * c + i * g
        return o * math.tanh(cn), cn, (i, f, g, o)
    h0, c0, g0 = step(x[0], 0.0, 0.0)
    h1, c1, g1 = step(x[1], h0, c0)
    u = [0.0, h0 * e[1], h1 * e[2]]
    loss = -sum(math.log(sg(v)) for v in u)
    gam = [-sg(-v) for v in u]                                # n = 1
    # backward, step 1 then step 0
    dh1 = gam[2] * e[2]
    i, f, g, o = g1; tc = math.tanh(c1)
    dc = dh1 * o * (1 - tc * tc)
    da1 = [dc * g * i * (1 - i), dc * c0 * f * (1 - f), dc * i * (1 - g * g), dh1 * tc * o * (1 - o)]
    dc0 = dc * f
    dh0 = sum(W[k] * da1[k] for k in range(4)) + gam[1] * e[1]
    dx1 = sum(U[k] * da1[k] for k in range(4))
    i, f, g, o = g0; tc = math.tanh(c0)
    dc = dc0 + dh0 * o * (1 - tc * tc)
    da0 = [dc * g * i * (1 - i), 0.0, dc * i * (1 - g * g), dh0 * tc * o * (1 - o)]
    dx0 = sum(U[k] * da0[k] for k in range(4))
    dU = [da0[k] * x[0] + da1[k] * x[1] for k in range(4)]
    dW = [da1[k] * h0 for k in range(4)]                      # h_{-1} = 0
    dB = [da0[k] + da1[k] for k in range(4)]
    dlt = np.zeros(5)
    dlt[p[0]] += dx0; dlt[p[1]] += dx1 + gam[1] * h0; dlt[q[1]] -= gam[1] * h0; dlt[p[2]] += gam[2] * h1; dlt[q[2]] -= gam[2] * h1
    len_max = 5
    mult = np.bincount(p + q + [4] * (2 * (len_max - 3)), minlength=5)
    P = dict(lt=lt, ui=ui, wh=wh, bi=bi)
    pm = np.array([p + [4, 4]]); qm = np.array([q + [4, 4]]); mm = np.array([[1, 1, 1, 0, 0]])
    got, got_loss = C.minibatch_step(P, pm, qm, mm, ALPHA, LAM, "lstm")
    assert abs(got_loss - loss) < 1e-14
    assert np.allclose(got["ui"].ravel(), U - ALPHA * (np.array(dU) + LAM * U), rtol=0, atol=1e-15)
    assert np.allclose(got["wh"].ravel(), W - ALPHA * (np.array(dW) + LAM * W), rtol=0, atol=1e-15)
    assert np.allclose(got["bi"].ravel(), B - ALPHA * (np.array(dB) + LAM * B), rtol=0, atol=1e-15)
    assert np.allclose(got["lt"].ravel(), lt.ravel() - ALPHA * (dlt + LAM * mult * lt.ravel()), rtol=0, atol=1e-15)
    assert mult[4] == 4 and got["lt"][4, 0] != lt[4, 0]       # the pad row decays although no position of the user names it


def test_predict_runs_every_position():
    P = _params(9, 10, 4, "lstm")
    pm, _, mm = _batch(1, 2, 10, 5, [5, 2])
    h = C.predict(P, pm, mm, "lstm")
    hh, cc = np.zeros(4), np.zeros(4)
    for t in range(2):
        hh, cc, _ = C.cell_step(P, "lstm", P["lt"][pm[1, t]], hh, cc)
    assert np.array_equal(h[1], hh) and h.shape == (2, 4)
