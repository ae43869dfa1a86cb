"""Float64 numpy restatement of the reference's mini-batch `Lstm` (public/GRU.py:502-657) and `Rnn` (:661-809): the oracle of
tests/test_gpu_cells.py, itself held to torch-autograd of a literal transcription of the reference graph in tests/test_cells_cpu.py.

The reference scans every user of a batch to the batch's longest length and feeds pad rows to the shorter ones; those steps carry no
loss and nothing reads their states, so a user needs exactly L - 1 cell steps.  What the padding does change is the L2 term: every
one of the n x len_max gathered positions of p and of q counts, pad rows and duplicates included.  Here every user is walked on its
own (`sequence_grads`, L - 1 steps) and the pad touches are counted analytically (`multiplicities`)."""
import numpy as np

CELLS = ("lstm", "rnn")


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def log_sigmoid(x):
    return np.where(x >= 0, -np.log1p(np.exp(-np.abs(x))), x - np.log1p(np.exp(-np.abs(x))))


def init_params(rng, n_item, dim, cell):
    """The reference's init (GRU.py:506-510, :665-668): uniform(-0.5, 0.5) tables and weights, zero bias."""
    g = (4,) if cell == "lstm" else ()
    u = lambda *s: rng.uniform(-0.5, 0.5, s)
    return dict(lt=u(n_item + 1, dim), ui=u(*g, dim, dim), wh=u(*g, dim, dim), bi=np.zeros(g + (dim,)))


def cell_step(P, cell, x, h, c):
    """-> (h_t, c_t, cache) of one cell step on float64 vectors."""
    if cell == "rnn":
        hn = sigmoid(P["ui"] @ x + P["wh"] @ h + P["bi"])
        return hn, c, (x, h, hn)
    a = P["ui"] @ x + P["wh"] @ h + P["bi"]                   # (4, D)
    i, f, g, o = sigmoid(a[0]), sigmoid(a[1]), np.tanh(a[2]), sigmoid(a[3])
    cn = f * c + i * g
    tc = np.tanh(cn)
    return o * tc, cn, (x, h, c, i, f, g, o, tc)


def sequence_grads(P, p, q, cell, n=1):
    """One user with positions p, q (length L, unpadded): loss = -sum_t log sigmoid(h_{t-1} . (lt[p_t] - lt[q_t])) and the gradients
    of loss / n: (loss, d ui, d wh, d bi, rows, d rows) with one (row, vector) pair per touch, duplicates not merged."""
    lt = P["lt"]
    L, D = len(p), lt.shape[1]
    h, c = np.zeros(D), np.zeros(D)
    hs, caches, gam = [], [], np.zeros(L)
    loss = 0.0
    for t in range(L):
        e = lt[p[t]] - lt[q[t]]
        u = h @ e
        loss -= float(log_sigmoid(u))
        gam[t] = -sigmoid(-u) / n
        hs.append(h)
        if t < L - 1:
            h, c, cache = cell_step(P, cell, lt[p[t]], h, c)
            caches.append(cache)
    G = {k: np.zeros_like(P[k]) for k in ("ui", "wh", "bi")}
    rows, vecs = [], []
    for t in range(L):
        rows += [p[t], q[t]]
        vecs += [gam[t] * hs[t], -gam[t] * hs[t]]
    dh = gam[L - 1] * (lt[p[L - 1]] - lt[q[L - 1]])
    dc = np.zeros(D)
    for t in range(L - 2, -1, -1):
        if cell == "rnn":
            x, hp, hn = caches[t]
            da = dh * hn * (1.0 - hn)
            G["ui"] += np.outer(da, x); G["wh"] += np.outer(da, hp); G["bi"] += da
            dx, dhp = P["ui"].T @ da, P["wh"].T @ da
        else:
            x, hp, cp, i, f, g, o, tc = caches[t]
            dc = dc + dh * o * (1.0 - tc * tc)
            da = np.stack([dc * g * i * (1.0 - i), dc * cp * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)])
            dc = dc * f
            G["ui"] += da[:, :, None] * x[None, None, :]; G["wh"] += da[:, :, None] * hp[None, None, :]; G["bi"] += da
            dx, dhp = np.einsum("gjd,gj->d", P["ui"], da), np.einsum("gjd,gj->d", P["wh"], da)
        rows.append(p[t]); vecs.append(dx)
        dh = dhp + gam[t] * (lt[p[t]] - lt[q[t]])
    return loss, G["ui"], G["wh"], G["bi"], np.asarray(rows), np.asarray(vecs)


def multiplicities(p_rows, q_rows, n_rows):
    """L2 multiplicity of every POI row: its count over ALL len_max positions of p and of q of all users (pad positions hold n_item)."""
    return np.bincount(np.concatenate((np.asarray(p_rows).ravel(), np.asarray(q_rows).ravel())), minlength=n_rows).astype(np.float64)


def minibatch_step(P, p_rows, q_rows, masks, alpha, lam, cell):
    """seq_train(start_end) on padded (n, len_max) tables -> (new parameters, -sum of log sigmoid over the batch).
    dense: theta -= alpha (G / n + lam theta); rows of unique(p U q): row -= alpha (G_row / n + lam mult row)."""
    p_rows, q_rows, masks = (np.asarray(a) for a in (p_rows, q_rows, masks))
    n = len(p_rows)
    G = {k: np.zeros_like(np.asarray(P[k], np.float64)) for k in ("lt", "ui", "wh", "bi")}
    total = 0.0
    for k in range(n):
        L = int(masks[k].sum())
        loss, dui, dwh, dbi, rows, vecs = sequence_grads(P, p_rows[k, :L], q_rows[k, :L], cell, n)
        total += loss
        G["ui"] += dui; G["wh"] += dwh; G["bi"] += dbi
        np.add.at(G["lt"], rows, vecs)
    mult = multiplicities(p_rows, q_rows, P["lt"].shape[0])
    N = dict(P)
    for k in ("ui", "wh", "bi"):
        N[k] = P[k] - alpha * (G[k] + lam * P[k])
    N["lt"] = P["lt"] - alpha * (G["lt"] + lam * mult[:, None] * P["lt"])
    return N, total


def predict(P, p_rows, masks, cell):
    """seq_predict(start_end): h_{L-1} per user, the cell over all L positions."""
    D = P["lt"].shape[1]
    out = np.zeros((len(p_rows), D))
    for k in range(len(p_rows)):
        h, c = np.zeros(D), np.zeros(D)
        for t in range(int(np.asarray(masks[k]).sum())):
            h, c, _ = cell_step(P, cell, P["lt"][p_rows[k][t]], h, c)
        out[k] = h
    return out
