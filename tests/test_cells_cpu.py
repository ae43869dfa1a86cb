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


# ---- the batched oracle and the launch-size cases (tests/cells_cases.py, tests/test_gpu_cells_launch_sizes.py) -------------------------
from tests import cells_cases as K                                                 # noqa: E402
from tests.gpu_util import delta_excess                                            # noqa: E402

RAGGED = [("ragged", [9, 1, 2, 5, 7, 3, 2, 9], 9), ("short_only", [1, 2, 1, 2], 5), ("one_user_len1", [1], 4), ("padded_beyond_longest", [6, 2, 4], 8)]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("dim", [4, 20])
@pytest.mark.parametrize("name,lens,len_max", RAGGED, ids=[c[0] for c in RAGGED])
def test_batched_oracle_equals_the_loop(cell, dim, name, lens, len_max):
    """Float64 against float64, the users' terms added in another order: the new tables, what the step changed and the loss agree to
    1e-12 relative (measured: below 1e-15 on the tables, at most 8.2e-14 on the updates, which are a hundredth of the tables)."""
    n_item = 17
    P = _params(21, n_item, dim, cell)
    pm, qm, mm = _batch(6, len(lens), n_item, len_max, lens)
    ref, ref_loss = C.minibatch_step(P, pm, qm, mm, ALPHA, LAM, cell)
    got, loss = C.minibatch_step_batched(P, pm, qm, mm, ALPHA, LAM, cell)
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss), (loss, ref_loss)
    worst = 0.0
    for k in ("lt", "ui", "wh", "bi"):
        assert got[k].shape == ref[k].shape
        e_w, e_d = _rel(got[k], ref[k]), _rel(got[k] - P[k], ref[k] - P[k])
        worst = max(worst, e_d)
        assert e_w <= 1e-12 and e_d <= 1e-12, (k, e_w, e_d)
    print("batched vs loop %s dim %d %s: worst update error %.2e" % (cell, dim, name, worst))
    assert np.array_equal(got["lt"] != P["lt"], ref["lt"] != P["lt"])            # the same rows move
    h_ref, h_got = C.predict(P, pm, mm, cell), C.predict_batched(P, pm, mm, cell)
    assert h_got.shape == h_ref.shape and _rel(h_got, h_ref) <= 1e-12


def test_sort_passes_mirror_and_case_preconditions():
    assert [K.sort_passes(v) for v in K.A_N_ITEM] == list(K.A_PASSES)
    assert [K.sort_passes(v) for v in (1, 70, 100_000, (1 << 27) - 2, (1 << 27) - 1)] == [1, 1, 2, 3, 4]
    assert [K.chunk_rows(n, m) for n, m in ((1, 1), (64, 50), (257, 11), (5300, 50))] == [8, 56, 48, 4144]
    for n_item in K.A_N_ITEM:
        rag, full = K.case_a(n_item, False), K.case_a(n_item, True)
        u = np.arange(40)
        assert K.pad_multiplicity(rag, u) > 0 and K.pad_multiplicity(full, u) == 0
        for c in (rag, full):
            pm, mm, qm = c["train"]
            assert pm[mm > 0].min() == 0 and qm[mm > 0].max() >= n_item - 1 and max(pm.max(), qm.max()) <= n_item
        assert (full["train"][0] == n_item).sum() == 0 and (full["train"][2] == n_item).sum() == 0
        assert (rag["train"][2][rag["train"][1] > 0] == n_item).sum() == 1      # the pad row as a real negative
    b = K.case_b()
    for n in K.B_SIZES:
        lens = b["lens"][K.b_users(b, n)]
        assert lens[255 if n > 255 else 0] == (1 if n > 255 else lens[0]) and (n <= 256 or lens[256] == 1)
    assert K.position_rows(b, K.b_users(b, 257)) % K.chunk_rows(257, K.max_len(b)) != 0
    assert K.pad_multiplicity(b, K.b_users(b, 769)) < 3000
    c1 = K.case_c1()
    assert K.sort_entries(c1, np.arange(513)) > K.COMMIT_GRID_MAX
    c2 = K.case_c2()
    assert K.max_len(c2) == 50 and K.position_rows(c2, np.arange(64)) < 2 * K.chunk_rows(64, 50)
    lens = np.full(K.D_N_USER, 50); lens[-1] = 49                               # case D without building its tables
    assert lens.sum() > 262144 and -(-(2 * lens.sum() + 1) // 64) > K.WINDOW_GRID_MAX and K.sort_passes(K.D_N_ITEM) == 3
    assert -(-(2 * (lens.sum() - 100 * 50) + 1) // 64) <= K.WINDOW_GRID_MAX     # 5200 users stay under the cap


def _verdict(got_lt, exp_lt, old_lt, touched):
    """What tests/test_gpu_cells_launch_sizes.py asserts on lt: (delta excess, rows the oracle leaves alone that moved)."""
    return delta_excess(got_lt, exp_lt, old_lt)[0], int((got_lt[~touched] != old_lt[~touched]).any(axis=1).sum())


def _flagged(v):
    return v[0] > 1.0 or v[1] > 0


@pytest.fixture(scope="module", params=C.CELLS)
def replica(request):
    """Case D reduced to 530 users (three plan blocks, three sort passes, the same 50-position users and 262 143 POIs) and its gradients."""
    cell = request.param
    case = K.case_d(530)
    P = K.params(90, K.D_N_ITEM, 8, cell)
    pm, qm, mm = K.tables(case, np.arange(530))
    losses, G, rows, vecs, ent = C.batch_grads(P, pm, qm, mm, cell)
    mult = C.multiplicities(pm, qm, P["lt"].shape[0])
    exp = C.apply_grads(P, G, rows, vecs, mult, ALPHA, LAM)["lt"]
    return dict(P=P, G=G, rows=rows, vecs=vecs, ent=ent, mult=mult, exp=exp, touched=mult > 0, pm=pm, qm=qm, case=case)


def _corrupt(R, rows=None, vecs=None, mult=None):
    lt = C.apply_grads(R["P"], R["G"], R["rows"] if rows is None else rows, R["vecs"] if vecs is None else vecs,
                       R["mult"] if mult is None else mult, ALPHA, LAM)["lt"]
    return _verdict(lt, R["exp"], R["P"]["lt"], R["touched"])


def _single_touch_entries(R, side):
    """Sorted entries (of the positives: side 0, the negatives: side 1) that are the only touch of their row, weakest gradient first."""
    keep = np.flatnonzero((R["mult"][R["rows"]] == 1) & (R["ent"] % 2 == side))
    mass = np.zeros(int(R["ent"].max()) + 1)
    np.maximum.at(mass, R["ent"][keep], np.abs(R["vecs"][keep]).max(axis=1))
    ents = np.unique(R["ent"][keep])
    return ents[np.argsort(mass[ents], kind="stable")]


def test_replica_is_sparse_and_clean(replica):
    R = replica
    assert (R["mult"][R["touched"]] == 1).mean() > 0.8                          # most touched rows hold one sorted entry
    assert R["mult"][R["case"]["hot"]].min() > 4 * K.WINDOW                    # the planted hot POIs cross several windows each
    assert R["mult"][0] >= 1 and R["mult"][K.D_N_ITEM - 1] >= 1 and R["mult"][K.D_N_ITEM] == 3      # 2 analytic + the planted negative
    assert _corrupt(R) == (0.0, 0)


@pytest.mark.parametrize("pick", ["weakest", "median", "strongest"])
def test_a_dropped_single_touch_entry_is_flagged(replica, pick):
    """(a) one sorted entry lost from a row it alone touches: its gradient and its unit of L2 multiplicity are gone, the row stays put.
    Also for the weakest such entry, a negative at t = 0 whose gradient is exactly zero (h_{-1} = 0): its L2 term alone is 40x over."""
    R = replica
    ents = _single_touch_entries(R, 1)
    e = ents[{"weakest": 0, "median": len(ents) // 2, "strongest": -1}[pick]]
    keep = R["ent"] != e
    mult = R["mult"].copy()
    mult[R["rows"][~keep][0]] -= 1
    v = _corrupt(R, R["rows"][keep], R["vecs"][keep], mult)
    print("(a) %s entry dropped: excess %.1f" % (pick, v[0]))
    assert v[0] > 1.0


def test_an_entry_credited_to_the_next_row_is_flagged(replica):
    """(b) a positive's entry (gam h and ui^T da) lands on row r + 1: row r loses its update, row r + 1 - untouched in the oracle - moves."""
    R = replica
    for e in _single_touch_entries(R, 0):
        sel = R["ent"] == e
        r = int(R["rows"][sel][0])
        if r + 1 < K.D_N_ITEM and R["mult"][r + 1] == 0:
            break
    rows, mult = R["rows"].copy(), R["mult"].copy()
    rows[sel] += 1
    mult[r] -= 1; mult[r + 1] += 1
    v = _corrupt(R, rows=rows, mult=mult)
    print("(b) entry on row r + 1: excess %.1f, untouched rows moved %d" % v)
    assert v[0] > 1.0 and v[1] == 1


def test_a_user_of_the_second_plan_block_contributing_nothing_is_flagged(replica):
    """(d) user 300 of the launch (second block of 256 of cell_plan_kernel's scan) leaves no row entry."""
    R = replica
    user = R["ent"] // (2 * R["case"]["len_max"])
    keep = user != 300
    mult = R["mult"] - np.bincount(np.concatenate((R["pm"][300], R["qm"][300])), minlength=len(R["mult"]))
    v = _corrupt(R, R["rows"][keep], R["vecs"][keep], mult)
    print("(d) user 300 silent: excess %.1f" % v[0])
    assert v[0] > 1.0


def _pad_off_by_one(case, idxs, cell, seed):
    P = K.params(seed, case["n_item"], case["dim"], cell)
    pm, qm, mm = K.tables(case, idxs)
    losses, G, rows, vecs, _ = C.batch_grads(P, pm, qm, mm, cell)
    mult = C.multiplicities(pm, qm, P["lt"].shape[0])
    exp = C.apply_grads(P, G, rows, vecs, mult, ALPHA, LAM)["lt"]
    out = []
    for d in (1, -1):
        bad = mult.copy()
        bad[case["n_item"]] += d
        if bad[case["n_item"]] >= 0:
            out.append(_verdict(C.apply_grads(P, G, rows, vecs, bad, ALPHA, LAM)["lt"], exp, P["lt"], mult > 0))
    return mult[case["n_item"]], out


def _assert_flagged(seen):
    for what, m, v in seen:
        print("(c) %s, pad multiplicity %d off by one: excess %.2f, untouched rows moved %d" % (what, m, v[0], v[1]))
        assert m < 1e4 and _flagged(v), (what, m, v)


@pytest.mark.parametrize("cell", C.CELLS)
def test_pad_multiplicity_off_by_one_is_flagged(cell):
    """(c) on case A (ragged: the delta bar; full length: the pad row is untouched and must not move) and on case B's largest launch,
    where the multiplicity is largest and the bar weakest: 1e-4 of an update of alpha lambda mult |row| against a shift of
    alpha lambda |row| - the excess falls as 1e4 / mult, so the cases keep mult well below 1e4."""
    seen = []
    for n_item in (K.A_N_ITEM[0], K.A_N_ITEM[-1]):
        for full in (False, True):
            m, vs = _pad_off_by_one(K.case_a(n_item, full), np.arange(40), cell, 1)
            assert (m == 0) == full
            seen += [("A %d %s" % (n_item, "full" if full else "ragged"), m, v) for v in vs]
    b = K.case_b()
    m, vs = _pad_off_by_one(b, K.b_users(b, 769), cell, 2)
    _assert_flagged(seen + [("B 769", m, v) for v in vs])


def test_pad_multiplicity_off_by_one_is_flagged_on_the_replica(replica):
    R, seen = replica, []
    for d in (1, -1):
        bad = R["mult"].copy()
        bad[K.D_N_ITEM] += d
        seen.append(("D replica %+d" % d, R["mult"][K.D_N_ITEM], _corrupt(R, mult=bad)))
    _assert_flagged(seen)
