"""Float64 restatement of PRME (public/PRME.py, OboPrme) for the tests: the one-transition step with Theano's last-wins collapse, the
project's capped snapshot rule over a launch of transitions (include/poi_hip.h, "Batch semantics"), the scoring rows and l2.  numpy only.

Quirks kept from the reference (both are what CPU Theano computes):
  1. dp[prev] - and in the far branch (gap > threshold) all three ds rows - get the L2 decay although they are not in the loss;
  2. set_subtensor with a repeated index keeps the LAST occurrence in the order (p, q, prev): with p == prev, dp[p] moves by decay only
     and ds[p] takes the prev occurrence's update.  After the collapse each distinct row is one touch of its transition."""
import numpy as np

TABLES = ("du", "dp", "ds")


def init_tables(rng, n_user, n_item, dim):
    """uniform(-0.5, 0.5) tables of PRME.py:75-78: du (n_user, D); dp, ds (n_item + 1, D)."""
    u = lambda *s: rng.uniform(-0.5, 0.5, s)
    return dict(du=u(n_user, dim), dp=u(n_item + 1, dim), ds=u(n_item + 1, dim))


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def transition_terms(P, u, p, q, prev, d, gap, alpha, lam, thd=360, cw=0.2):
    """(loss, [(table, row, delta)]) of one transition at the values in P, after the last-wins collapse (deltas in the order the
    reference assigns them: du; dp p, q, prev; ds p, q, prev - a later entry for the same row replaces the earlier one)."""
    far = gap > thd
    w = (1.0 + d) ** 0.25
    a, b = (1.0, 0.0) if far else (w * cw, w * (1.0 - cw))
    U, Pp, Pq, Pv = P["du"][u], P["dp"][p], P["dp"][q], P["dp"][prev]
    Sp, Sq, Sv = P["ds"][p], P["ds"][q], P["ds"][prev]
    Dp = a * ((U - Pp) ** 2).sum() + b * ((Sp - Sv) ** 2).sum()
    Dq = a * ((U - Pq) ** 2).sum() + b * ((Sq - Sv) ** 2).sum()
    x = Dq - Dp
    g = _sig(-x)
    loss = np.log(_sig(x))
    terms = [("du", u, alpha * (g * 2 * a * (Pp - Pq) - lam * U)),
             ("dp", p, alpha * (g * 2 * a * (U - Pp) - lam * Pp)),
             ("dp", q, alpha * (-g * 2 * a * (U - Pq) - lam * Pq)),
             ("dp", prev, alpha * (-lam * Pv)),
             ("ds", p, alpha * (-g * 2 * b * (Sp - Sv) - lam * Sp)),
             ("ds", q, alpha * (g * 2 * b * (Sq - Sv) - lam * Sq)),
             ("ds", prev, alpha * (g * 2 * b * (Sp - Sq) - lam * Sv))]
    last = {}
    for tb, r, v in terms:
        last[(tb, int(r))] = v
    return loss, [(tb, r, v) for (tb, r), v in last.items()]


def step(P, u, p, q, prev, d, gap, alpha, lam, thd=360, cw=0.2):
    """The reference step on a copy of P: (new tables, loss)."""
    loss, dl = transition_terms(P, u, p, q, prev, d, gap, alpha, lam, thd, cw)
    Q = {k: v.copy() for k, v in P.items()}
    for t, r, v in dl:
        Q[t][r] += v
    return Q, loss


def is_bad(P, u, p, q, prev, d):
    n_user, rows = len(P["du"]), len(P["dp"])
    return not (0 <= u < n_user and all(0 <= x < rows for x in (p, q, prev))) or p == q or not np.isfinite(d) or d < 0


def batch_step(P, u, p, q, prev, d, gap, alpha, lam, cap=1.0, thd=360, cw=0.2, absmass=False):
    """A launch under the snapshot rule: every transition's (collapsed) deltas at the launch-entry values; a row touched k times moves by
    min(k, cap) / k times the sum of its deltas.  Rejected transitions contribute nothing and get a NaN loss.  With absmass, also the same
    combination of the deltas' absolute values (the per-row scale of gpu_util.delta_excess)."""
    sums = {k: np.zeros_like(v) for k, v in P.items()}
    mass = {k: np.zeros_like(v) for k, v in P.items()}
    cnt = {k: np.zeros(len(v), np.int64) for k, v in P.items()}
    losses = np.full(len(u), np.nan)
    for t in range(len(u)):
        args = (int(u[t]), int(p[t]), int(q[t]), int(prev[t]), float(d[t]))
        if is_bad(P, *args):
            continue
        losses[t], dl = transition_terms(P, *args, int(gap[t]), alpha, lam, thd, cw)
        for tb, r, v in dl:
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


def cal_dis(lat1, lon1, lat2, lon2):
    """public/Load_Data_prme.py:24-35 in float64."""
    rad = lambda x: np.multiply(np.asarray(x, np.float64), np.pi) / 180.0
    r1, r2 = rad(lat1), rad(lat2)
    a, b = r1 - r2, rad(lon1) - rad(lon2)
    return 2 * np.arcsin(np.sqrt(np.sin(a / 2) ** 2 + np.cos(r1) * np.cos(r2) * np.sin(b / 2) ** 2)) * 6378.137


def score_rows(P, coords, users, qpoi, cw=0.2):
    """compute_sub_all_scores (PRME.py:117-139) for rows (users[r], qpoi[r]) against the candidates j < n_item: (n_rows, n_item) float64
    -(1 + cal_dis(l, j))^0.25 (cw |du_u - dp_j|^2 + (1 - cw) |ds_l - ds_j|^2).  P holds the trained snapshots; coords has the pad row."""
    n_item = len(coords) - 1
    users, qpoi = np.asarray(users), np.asarray(qpoi)
    U, S = P["du"][users], P["ds"][qpoi]
    dp, ds = P["dp"][:n_item], P["ds"][:n_item]
    Dp = ((U[:, None, :] - dp[None, :, :]) ** 2).sum(2)
    Ds = ((S[:, None, :] - ds[None, :, :]) ** 2).sum(2)
    w = (1.0 + cal_dis(coords[qpoi, 0][:, None], coords[qpoi, 1][:, None], coords[None, :n_item, 0], coords[None, :n_item, 1])) ** 0.25
    return -w * (cw * Dp + (1.0 - cw) * Ds)


def reference_rows(off, tra_p, tes_p, tes_mask, users, n_item):
    """The reference's (user, query POI) layout of one evaluation batch (PRME.py:118-120): per user, column 0 queries the last train
    POI, columns t = 1 .. Lb-1 the test POI t-1 (the pad POI n_item beyond the user's list), Lb = the batch's longest test list."""
    users = np.asarray(users)
    lb = max(1, int(np.asarray(tes_mask)[users].sum(axis=1).max()))
    last = np.asarray(tra_p)[np.asarray(off, np.int64)[users + 1] - 1]
    q = np.full((len(users), lb), n_item, np.int64)
    q[:, 0] = last
    tp = np.asarray(tes_p)[users][:, :lb - 1]
    q[:, 1:1 + tp.shape[1]] = tp
    return np.repeat(users, lb), q.reshape(-1), lb


def l2(P, lam):
    """model.l2 (PRME.py:165-168): 0.5 lambda times the sum of squares of the three whole tables."""
    return 0.5 * lam * sum(float((P[k] ** 2).sum()) for k in TABLES)


def topk_desc(sc, k):
    """Rows' k best ids: descending score, then ascending id."""
    return np.stack([np.lexsort((np.arange(len(r)), -r))[:k] for r in np.asarray(sc)])
