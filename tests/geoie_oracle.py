"""Float64 numpy restatement of the GeoIE step (public/GeoIE.py:129-188) under the engine's rule for the reference's undefined cases
(include/poi_hip.h), the capped batch rule over a launch, the user vectors of the scoring and l2.

A user is a pair of int arrays (p, q) of its L train POIs and negatives; rows i = 0 .. L-2 target p[i+1] / q[i+1], columns j <= i."""
import numpy as np

from poi_amd.data import geoie_cal_dis

TABLES = ("g", "h", "t", "z")


def init_tables(rng, n_user, n_item, dim):
    """uniform(-0.5, 0.5) in the reference's order (GeoIE.py:65-75): g, h, t, z, then a, b."""
    P = dict(g=rng.uniform(-0.5, 0.5, (n_item + 1, dim)), h=rng.uniform(-0.5, 0.5, (n_item + 1, dim)),
             t=rng.uniform(-0.5, 0.5, (n_user, dim)), z=rng.uniform(-0.5, 0.5, (n_item + 1, dim)))
    P["a"] = float(rng.uniform(-0.5, 0.5))
    P["b"] = float(rng.uniform(-0.5, 0.5))
    return P


def round_f32(P):
    """The device tables are float32 (a, b float64): the oracle starts from the rounded values."""
    return {k: (np.asarray(v, np.float32).astype(np.float64) if k in TABLES else float(v)) for k, v in P.items()}


def pair_dists(coords, p, q):
    """(R, R) float32 dp, dq (zero above the diagonal), R = L - 1."""
    xy = np.asarray(coords, np.float64)
    R = len(p) - 1
    dp, dq = np.zeros((R, R), np.float32), np.zeros((R, R), np.float32)
    if R <= 0:
        return dp, dq
    ii, jj = np.tril_indices(R)
    s, tp, tq = xy[p[jj]], xy[p[ii + 1]], xy[q[ii + 1]]
    dp[ii, jj] = geoie_cal_dis(s[:, 0], s[:, 1], tp[:, 0], tp[:, 1])
    dq[ii, jj] = geoie_cal_dis(s[:, 0], s[:, 1], tq[:, 0], tq[:, 1])
    return dp, dq


def _f(d32, a, b, d_min, mask):
    """f = a d_eff^b, df/da, df/db on the masked pairs; bad where d_eff = 0 and b <= 0."""
    d = np.maximum(np.asarray(d32, np.float64), d_min)
    zero = mask & (d == 0.0)
    bad = bool(zero.any() and not b > 0)
    ok = mask & (d > 0.0)
    f, fa, fb = (np.zeros(d.shape) for _ in range(3))
    with np.errstate(all="ignore"):
        pw = np.where(ok, np.where(ok, d, 1.0) ** b, 0.0)
        f[ok] = a * pw[ok]
        fa[ok] = pw[ok]
        fb[ok] = a * pw[ok] * np.log(d[ok])
    return f, fa, fb, bad


def user_grads(P, p, q, coords, d_min=0.0):
    """One user's contribution at the values P: dict(loss, ok, rows (bool: L >= 2), da, db, G = {table: {row: loss gradient}},
    mult = {table: {row: occurrences}}).  G and da / db are derivatives of the cost (-loss + L2; the L2 part is lambda mult row)."""
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    n_item = P["g"].shape[0] - 1
    L = len(p)
    out = dict(loss=0.0, ok=True, rows=L >= 2, da=0.0, db=0.0, G={k: {} for k in TABLES}, mult={k: {} for k in TABLES})
    if L < 2:
        return out
    R = L - 1
    if p.min() < 0 or p.max() >= n_item or q[1:].min() < 0 or q[1:].max() >= n_item:
        out.update(ok=False, loss=float("nan"))
        return out
    a, b = P["a"], P["b"]
    Gp, HP, HQ = P["g"][p[:R]], P["h"][p[1:]], P["h"][q[1:]]
    M = np.tril(np.ones((R, R), bool))
    dp, dq = pair_dists(coords, p, q)
    Fp, Fpa, Fpb, bad1 = _f(dp, a, b, d_min, M)
    Fq, Fqa, Fqb, bad2 = _f(dq, a, b, d_min, M)
    X, Y = HP @ Gp.T, HQ @ Gp.T
    n_h = np.arange(1, R + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        diff = (X * Fp - Y * Fq).sum(1) / n_h
        c = 1.0 / (1.0 + np.exp(diff)) / n_h
        loss = float(-np.logaddexp(0.0, -diff).sum())
        g_hp = -c[:, None] * (Fp @ Gp)
        g_hq = c[:, None] * (Fq @ Gp)
        g_g = -((c[:, None] * Fp).T @ HP - (c[:, None] * Fq).T @ HQ)
        da = float(-(c * (X * Fpa - Y * Fqa).sum(1)).sum())
        db = float(-(c * (X * Fpb - Y * Fqb).sum(1)).sum())
    finite = all(np.all(np.isfinite(v)) for v in (diff, g_hp, g_hq, g_g)) and np.isfinite([loss, da, db]).all()
    if bad1 or bad2 or not finite:
        out.update(ok=False, loss=float("nan"))
        return out
    G, mult = out["G"], out["mult"]

    def add(tab, row, vec):
        row = int(row)
        G[tab][row] = G[tab].get(row, 0.0) + vec
        mult[tab][row] = mult[tab].get(row, 0) + 1

    D = P["g"].shape[1]
    for j in range(R):
        add("g", p[j], g_g[j])
    for i in range(R):
        add("h", p[i + 1], g_hp[i]); add("h", q[i + 1], g_hq[i])
        add("z", p[i + 1], np.zeros(D)); add("z", q[i + 1], np.zeros(D))
    out.update(loss=loss, da=da, db=db)
    return out


def batch_step(P, seqs, coords, alpha, lam, d_min=0.0, cap=1.0, absmass=False):
    """A launch of users seqs = [(p, q), ...] at the values P: a row touched by k accepted users moves by
    -alpha min(k, cap) / k sum_u (G_u + lambda mult_u row); a, b by -alpha min(n, cap) / n sum_u d_u over the n accepted users with rows.
    Returns (Q, losses[, absmass per table])."""
    Q = {k: (np.array(v, np.float64) if k in TABLES else float(v)) for k, v in P.items()}
    M = {k: np.zeros_like(Q[k]) for k in TABLES}
    per = [user_grads(P, p, q, coords, d_min) for p, q in seqs]
    for tab in ("g", "h", "z"):
        acc, am, cnt = {}, {}, {}
        for o in per:
            if not o["ok"]:
                continue
            for row, gv in o["G"][tab].items():
                upd = gv + lam * o["mult"][tab][row] * P[tab][row]
                acc[row] = acc.get(row, 0.0) + upd
                am[row] = am.get(row, 0.0) + np.abs(upd)
                cnt[row] = cnt.get(row, 0) + 1
        for row, s in acc.items():
            k = cnt[row]
            sc = alpha * min(k, cap) / k
            Q[tab][row] = P[tab][row] - sc * s
            M[tab][row] = sc * am[row]
    acc_users = [o for o in per if o["ok"] and o["rows"]]
    if acc_users:
        n = len(acc_users)
        sc = alpha * min(n, cap) / n
        Q["a"] = P["a"] - sc * sum(o["da"] for o in acc_users)
        Q["b"] = P["b"] - sc * sum(o["db"] for o in acc_users)
    losses = np.array([o["loss"] for o in per])
    return (Q, losses, M) if absmass else (Q, losses)


def step(P, p, q, coords, alpha, lam, d_min=0.0):
    """The reference step of one user (n == 1): (Q, loss)."""
    Q, losses = batch_step(P, [(p, q)], coords, alpha, lam, d_min)
    return Q, float(losses[0])


def user_vectors(P, off, p, len_max, norm="reference"):
    """(n_user, 2 D) [t[u] | m_u] of compute_sub_all_scores (GeoIE.py:117-127)."""
    off = np.asarray(off, np.int64)
    n_item, D = P["g"].shape[0] - 1, P["g"].shape[1]
    out = np.zeros((len(off) - 1, 2 * D))
    for u in range(len(off) - 1):
        s = np.asarray(p[off[u]:off[u + 1]], np.int64)
        L = len(s)
        tot = P["g"][s].sum(0) if L else np.zeros(D)
        if norm == "reference":
            nh = float(s.sum() + (len_max - L) * n_item)
            m = tot / nh
        else:
            m = tot / L if L else np.zeros(D)
        out[u, :D], out[u, D:] = P["t"][u], m
    return out


def scores(P, uvec):
    """s[u, k] = t[u].z[k] + m_u.h[k] over k < n_item."""
    D = P["g"].shape[1]
    n_item = P["g"].shape[0] - 1
    return uvec[:, :D] @ P["z"][:n_item].T + uvec[:, D:] @ P["h"][:n_item].T


def l2(P, lam):
    """model.l2 of GeoIE.py:92-98: 0.5 lambda (|g|^2 + |h|^2 + |t|^2 + |z|^2 + a^2 + b^2)."""
    return 0.5 * lam * (sum(float((np.asarray(P[k]) ** 2).sum()) for k in TABLES) + P["a"] ** 2 + P["b"] ** 2)
