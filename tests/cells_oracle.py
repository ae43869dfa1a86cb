"""Float64 numpy restatement of the reference's mini-batch `Lstm` (public/GRU.py:502-657) and `Rnn` (:661-809): the oracle of
tests/test_gpu_cells.py, itself held to torch-autograd of a literal transcription of the reference graph in tests/test_cells_cpu.py.

The reference scans every user of a batch to the batch's longest length and feeds pad rows to the shorter ones; those steps carry no
loss and nothing reads their states, so a user needs exactly L - 1 cell steps.  What the padding does change is the L2 term: every
one of the n x len_max gathered positions of p and of q counts, pad rows and duplicates included.  Here every user is walked on its
own (`sequence_grads`, L - 1 steps) and the pad touches are counted analytically (`multiplicities`): `minibatch_step` / `predict` are
the definition.  `minibatch_step_batched` / `predict_batched` do the same arithmetic for all users of the batch at once, (n, D) arrays
per position with finished users masked - the oracle of the launches of tests/test_gpu_cells_launch_sizes.py that the loop would walk
for half a minute; tests/test_cells_cpu.py holds them to the loop at 1e-12 relative."""
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


def cell_step_batched(P, cell, x, h, c):
    """cell_step on (n, D) arrays, one user per row -> (h_t, c_t, cache)."""
    if cell == "rnn":
        hn = sigmoid(x @ P["ui"].T + h @ P["wh"].T + P["bi"])
        return hn, c, (x, h, hn)
    a = np.einsum("gjd,nd->ngj", P["ui"], x) + np.einsum("gjd,nd->ngj", P["wh"], h) + P["bi"]      # (n, 4, D)
    i, f, g, o = sigmoid(a[:, 0]), sigmoid(a[:, 1]), np.tanh(a[:, 2]), sigmoid(a[:, 3])
    cn = f * c + i * g
    tc = np.tanh(cn)
    return o * tc, cn, (x, h, c, i, f, g, o, tc)


def batch_grads(P, p_rows, q_rows, masks, cell):
    """sequence_grads of every user of a padded batch at once: all users advance one position per pass as (n, D) arrays, a user past
    its own length is masked out.  -> (losses (n,), {ui, wh, bi: gradient of sum(losses) / n}, rows (K,), vecs (K, D), ent (K,)):
    one (row, vector) pair per touch of lt, duplicates not merged, and the sorted entry it belongs to as csrc/cells.hip numbers them,
    ent = 2 (k len_max + t) + (0: the positive p_t, whose two pairs gam h and ui^T da share it; 1: the negative q_t) for user k of
    the batch.  Same arithmetic as sequence_grads; only the order in which the users' terms are added differs."""
    p_rows, q_rows, masks = (np.asarray(a) for a in (p_rows, q_rows, masks))
    lt = np.asarray(P["lt"], np.float64)
    n, D = p_rows.shape[0], lt.shape[1]
    L = masks.sum(axis=1).astype(np.int64)
    T = int(L.max())
    ent0 = 2 * np.arange(n) * p_rows.shape[1]
    h, c = np.zeros((n, D)), np.zeros((n, D))
    hs, es, caches = [], [], []
    gam = np.zeros((n, T))
    losses = np.zeros(n)
    for t in range(T):
        act = t < L
        pt, qt = np.where(act, p_rows[:, t], 0), np.where(act, q_rows[:, t], 0)
        e = lt[pt] - lt[qt]
        u = (h * e).sum(axis=1)
        losses -= np.where(act, log_sigmoid(u), 0.0)
        gam[:, t] = np.where(act, -sigmoid(-u) / n, 0.0)
        hs.append(h); es.append(e)
        if t < T - 1:
            hn, cn, cache = cell_step_batched(P, cell, lt[pt], h, c)
            step = (t < L - 1)[:, None]
            h, c = np.where(step, hn, h), np.where(step, cn, c)
            caches.append(cache)
    G = {k: np.zeros_like(np.asarray(P[k], np.float64)) for k in ("ui", "wh", "bi")}
    rows, vecs, ent = [], [], []
    for t in range(T):
        a = np.flatnonzero(t < L)
        gh = gam[a, t, None] * hs[t][a]
        rows += [p_rows[a, t], q_rows[a, t]]; vecs += [gh, -gh]; ent += [ent0[a] + 2 * t, ent0[a] + 2 * t + 1]
    dh, dc = np.zeros((n, D)), np.zeros((n, D))
    for t in range(T - 1, -1, -1):
        last = L - 1 == t
        dh[last] = gam[last, t, None] * es[t][last]
        dc[last] = 0.0
        step = t < L - 1
        if not step.any():
            continue
        m = step[:, None]
        if cell == "rnn":
            x, hp, hn = caches[t]
            da = np.where(m, dh * hn * (1.0 - hn), 0.0)
            G["ui"] += da.T @ x; G["wh"] += da.T @ hp; G["bi"] += da.sum(axis=0)
            dx, dhp = da @ P["ui"], da @ P["wh"]
        else:
            x, hp, cp, i, f, g, o, tc = caches[t]
            dcn = dc + dh * o * (1.0 - tc * tc)
            da = np.stack([dcn * g * i * (1.0 - i), dcn * cp * f * (1.0 - f), dcn * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], axis=1)
            da = np.where(m[:, None, :], da, 0.0)                                 # (n, 4, D)
            dc = np.where(m, dcn * f, dc)
            G["ui"] += np.einsum("ngj,nd->gjd", da, x); G["wh"] += np.einsum("ngj,nd->gjd", da, hp); G["bi"] += da.sum(axis=0)
            dx, dhp = np.einsum("gjd,ngj->nd", P["ui"], da), np.einsum("gjd,ngj->nd", P["wh"], da)
        a = np.flatnonzero(step)
        rows.append(p_rows[a, t]); vecs.append(dx[a]); ent.append(ent0[a] + 2 * t)
        dh = np.where(m, dhp + gam[:, t, None] * es[t], dh)
    return losses, G, np.concatenate(rows), np.concatenate(vecs), np.concatenate(ent)


def apply_grads(P, G, rows, vecs, mult, alpha, lam):
    """The SGD write-back of minibatch_step from the gradients of batch_grads: the row gradients go through one np.add.at."""
    glt = np.zeros_like(np.asarray(P["lt"], np.float64))
    np.add.at(glt, rows, vecs)
    N = dict(P)
    for k in ("ui", "wh", "bi"):
        N[k] = P[k] - alpha * (G[k] + lam * P[k])
    N["lt"] = P["lt"] - alpha * (glt + lam * np.asarray(mult, np.float64)[:, None] * P["lt"])
    return N


def minibatch_step_batched(P, p_rows, q_rows, masks, alpha, lam, cell):
    """minibatch_step with all users advanced together (batch_grads): the oracle of the launches too large for the per-sequence loop.
    tests/test_cells_cpu.py holds it to minibatch_step at 1e-12 relative."""
    losses, G, rows, vecs, _ = batch_grads(P, p_rows, q_rows, masks, cell)
    mult = multiplicities(p_rows, q_rows, np.asarray(P["lt"]).shape[0])
    return apply_grads(P, G, rows, vecs, mult, alpha, lam), float(losses.sum())


def touched_rows(p_rows, q_rows, n_rows):
    """Rows of lt a launch may move: every row named by any of the n x len_max positions of p or q (the pad row among them when a
    user is shorter than len_max)."""
    return multiplicities(p_rows, q_rows, n_rows) > 0


def predict_batched(P, p_rows, masks, cell):
    """predict with all users advanced together: a user stops at its own length."""
    p_rows, masks = np.asarray(p_rows), np.asarray(masks)
    lt = np.asarray(P["lt"], np.float64)
    n, D = p_rows.shape[0], lt.shape[1]
    L = masks.sum(axis=1).astype(np.int64)
    h, c = np.zeros((n, D)), np.zeros((n, D))
    for t in range(int(L.max())):
        act = t < L
        hn, cn, _ = cell_step_batched(P, cell, lt[np.where(act, p_rows[:, t], 0)], h, c)
        h, c = np.where(act[:, None], hn, h), np.where(act[:, None], cn, c)
    return h


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
