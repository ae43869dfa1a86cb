"""Float64 restatement of FPMC-LR (public/FPMC_LR.py) for the tests: the one-transition step, the project's capped snapshot rule over a
launch of transitions (include/poi_hip.h, "Batch semantics"), reference-order scoring and AUC preference.  numpy only."""
import numpy as np

TABLES = ("ui", "iu", "ia", "ai")


def init_tables(rng, n_user, n_item, dim):
    """uniform(-0.5, 0.5) tables of FPMC_LR.py:52-59: ui (n_user, D); iu, ia, ai (n_item + 1, D)."""
    u = lambda *s: rng.uniform(-0.5, 0.5, s)
    return dict(ui=u(n_user, dim), iu=u(n_item + 1, dim), ia=u(n_item + 1, dim), ai=u(n_item + 1, dim))


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def transition_terms(P, u, a, i, j, alpha, lam):
    """(loss, [(table, row, delta)]) of one transition at the values in P (FPMC_LR.py:113-151): x = ui[u].(iu[i]-iu[j]) + ai[a].(ia[i]-ia[j]),
    loss = log sigmoid(x), s = sigmoid(-x); every delta is alpha (s * partner - lambda * row) at the same values."""
    U, A = P["ui"][u], P["ai"][a]
    Ii, Ij, Ai, Aj = P["iu"][i], P["iu"][j], P["ia"][i], P["ia"][j]
    x = U @ (Ii - Ij) + A @ (Ai - Aj)
    s = _sig(-x)
    loss = np.log(_sig(x))
    d = [("ui", u, alpha * (s * (Ii - Ij) - lam * U)), ("ai", a, alpha * (s * (Ai - Aj) - lam * A)),
         ("iu", i, alpha * (s * U - lam * Ii)), ("iu", j, alpha * (-s * U - lam * Ij)),
         ("ia", i, alpha * (s * A - lam * Ai)), ("ia", j, alpha * (-s * A - lam * Aj))]
    return loss, d


def step(P, u, a, i, j, alpha, lam):
    """The reference step on a copy of P: (new tables, loss)."""
    loss, d = transition_terms(P, u, a, i, j, alpha, lam)
    Q = {k: v.copy() for k, v in P.items()}
    for t, r, v in d:
        Q[t][r] += v
    return Q, loss


def batch_step(P, u, a, i, j, alpha, lam, cap=1.0, absmass=False):
    """A launch of n transitions under the snapshot rule: every transition's update at the launch-entry values; a row touched k times
    (touches of one table counted together) moves by min(k, cap) / k times the sum of its updates.  Transitions with an id outside its
    table or i == j contribute nothing and get a NaN loss.  With absmass, also the same combination of the updates' absolute values
    (the per-row scale of gpu_util.delta_excess)."""
    n_user, n_rows = len(P["ui"]), len(P["iu"])
    sums = {k: np.zeros_like(v) for k, v in P.items()}
    mass = {k: np.zeros_like(v) for k, v in P.items()}
    cnt = {k: np.zeros(len(v), np.int64) for k, v in P.items()}
    losses = np.full(len(u), np.nan)
    for t in range(len(u)):
        if not (0 <= u[t] < n_user and all(0 <= x < n_rows for x in (a[t], i[t], j[t]))) or i[t] == j[t]:
            continue
        losses[t], d = transition_terms(P, int(u[t]), int(a[t]), int(i[t]), int(j[t]), alpha, lam)
        for tb, r, v in d:
            sums[tb][r] += v
            mass[tb][r] += np.abs(v)
            cnt[tb][r] += 1
    Q, M = {}, {}
    for k in P:
        k_ = cnt[k].astype(np.float64)
        f = np.where(k_ > 0, np.minimum(k_, cap) / np.maximum(k_, 1.0), 0.0)[:, None]
        Q[k] = P[k] + f * sums[k]
        M[k] = f * mass[k]
    return (Q, losses, M) if absmass else (Q, losses)


def scores(P, users, last):
    """FPMC_LR.py:76-82: score[u][k] = ui[u].iu[k] + ai[last(u)].ia[k] over the real POIs k < n_item."""
    return P["ui"][users] @ P["iu"][:-1].T + P["ai"][last[users]] @ P["ia"][:-1].T


def auc_preference(P, users, last, tes_p, tes_q, tes_m):
    """FPMC_LR.py:84-104 -> bool (n, len_tes)."""
    U, A = P["ui"][users], P["ai"][last[users]]
    up = (U[:, None, :] * (P["iu"][tes_p[users]] - P["iu"][tes_q[users]])).sum(2) + \
        (A[:, None, :] * (P["ia"][tes_p[users]] - P["ia"][tes_q[users]])).sum(2)
    return up * tes_m[users] > 0


def l2(P, lam):
    """model.l2 (FPMC_LR.py:66-69): 0.5 lambda sum of squares over the four whole tables."""
    return 0.5 * lam * sum(float((P[k] ** 2).sum()) for k in TABLES)
