"""Float64 numpy restatement of OboVBpr (public/BPR.py:245-335): the single step, the batch rule of include/poi_hip.h on top of it, the
evaluation snapshots [lt | fi ei^T] / [ux | ue] and l2.eval().  Parameters: dict(ux, lt, ue, ei) + the fixed feature table fi
((n_item + 1, F), pad row zero)."""
import numpy as np

NAMES = ("ux", "lt", "ue", "ei")


def init_params(rng, n_user, n_item, d, n_img):
    """public/BPR.py:50-54 and :251-257: uniform(-0.5, 0.5) everywhere."""
    u = lambda *s: rng.uniform(-0.5, 0.5, s)
    return dict(ux=u(n_user, d), lt=u(n_item + 1, d), ue=u(n_user, d), ei=u(d, n_img))


def margin(P, fi, u, p, q):
    """uij of :287-289 for arrays of triples -> (x, d = fi[p] - fi[q], v = ei d)."""
    d = fi[p] - fi[q]
    v = d @ P["ei"].T
    x = np.einsum("nd,nd->n", P["ux"][u], P["lt"][p] - P["lt"][q]) + np.einsum("nd,nd->n", P["ue"][u], v)
    return x, d, v


def step(P, fi, u, p, q, alpha, lam, lam_ev):
    """One bpr_train(u, [p, q]) call (:268-319) -> (new parameters, -log sigmoid(x)); every update at the old values."""
    P = {k: np.asarray(P[k], np.float64) for k in NAMES}
    fi = np.asarray(fi, np.float64)
    x, d, v = margin(P, fi, np.array([u]), np.array([p]), np.array([q]))
    x, d, v = float(x[0]), d[0], v[0]
    g = -1.0 / (1.0 + np.exp(x))
    N = {k: P[k].copy() for k in NAMES}
    N["ux"][u] = P["ux"][u] - alpha * (g * (P["lt"][p] - P["lt"][q]) + lam * P["ux"][u])
    N["ue"][u] = P["ue"][u] - alpha * (g * v + lam * P["ue"][u])
    N["lt"][p] = P["lt"][p] - alpha * (g * P["ux"][u] + lam * P["lt"][p])
    N["lt"][q] = P["lt"][q] - alpha * (-g * P["ux"][u] + lam * P["lt"][q])
    N["ei"] = P["ei"] - alpha * (g * np.outer(P["ue"][u], d) + lam_ev * P["ei"])
    return N, float(np.logaddexp(0.0, -x))


def accepted(P, u, p, q):
    n_user, n_item = P["ux"].shape[0], P["lt"].shape[0] - 1
    u, p, q = (np.asarray(a, np.int64) for a in (u, p, q))
    return (u >= 0) & (u < n_user) & (p >= 0) & (p <= n_item) & (q >= 0) & (q <= n_item) & (p != q)


def batch_step(P, fi, u, p, q, alpha, lam, lam_ev, cap):
    """A launch of n triples (include/poi_hip.h): every triple at the entry values; a row touched by k triples moves by min(k, cap) / k of
    their summed reference updates; ei by min(n_acc, cap) / n_acc of -alpha (sum_i g_i ue[u_i] (x) d_i + n_acc lambda_ev ei).  Rejected
    triples (accepted() false) move nothing and have loss NaN.  -> (new parameters, losses (n))."""
    P = {k: np.asarray(P[k], np.float64) for k in NAMES}
    fi = np.asarray(fi, np.float64)
    u, p, q = (np.asarray(a, np.int64) for a in (u, p, q))
    ok = accepted(P, u, p, q)
    loss = np.full(len(u), np.nan)
    ua, pa, qa = u[ok], p[ok], q[ok]
    N = {k: P[k].copy() for k in NAMES}
    if not len(ua):
        return N, loss
    x, d, v = margin(P, fi, ua, pa, qa)
    g = -1.0 / (1.0 + np.exp(x))
    loss[ok] = np.logaddexp(0.0, -x)
    G = {k: np.zeros_like(P[k]) for k in ("ux", "lt", "ue")}
    C = {k: np.zeros(P[k].shape[0]) for k in ("ux", "lt", "ue")}
    np.add.at(G["ux"], ua, g[:, None] * (P["lt"][pa] - P["lt"][qa])); np.add.at(C["ux"], ua, 1)
    np.add.at(G["ue"], ua, g[:, None] * v); np.add.at(C["ue"], ua, 1)
    np.add.at(G["lt"], pa, g[:, None] * P["ux"][ua]); np.add.at(C["lt"], pa, 1)
    np.add.at(G["lt"], qa, -g[:, None] * P["ux"][ua]); np.add.at(C["lt"], qa, 1)
    for k in ("ux", "lt", "ue"):
        c = C[k]
        sc = np.where(c > 0, alpha * np.minimum(c, cap), 0.0)
        N[k] = P[k] - sc[:, None] * (G[k] / np.maximum(c, 1)[:, None] + lam * P[k])
    na = float(len(ua))
    N["ei"] = P["ei"] - alpha * min(na, cap) * (((g[:, None] * P["ue"][ua]).T @ d) / na + lam_ev * P["ei"])
    return N, loss


def items(P, fi):
    """update_trained_items (:321-329): [lt | fi ei^T]."""
    return np.concatenate([np.asarray(P["lt"], np.float64), np.asarray(fi, np.float64) @ np.asarray(P["ei"], np.float64).T], axis=1)


def users(P):
    """update_trained_users (:331-335): [ux | ue]."""
    return np.concatenate([np.asarray(P["ux"], np.float64), np.asarray(P["ue"], np.float64)], axis=1)


def l2(P, lam, lam_ev):
    """l2.eval() (:259-265)."""
    sq = lambda k: float((np.asarray(P[k], np.float64) ** 2).sum())
    return 0.5 * lam * (sq("ux") + sq("lt") + sq("ue")) + 0.5 * lam_ev * sq("ei")
