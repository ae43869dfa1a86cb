"""Float64 numpy restatement of POI2Vec (public/POI2Vec.py, driver prog_poi2vec.py): the one-user step with its hand-derived gradients
(tests/test_poi2vec_cpu.py holds it to torch autograd of the reference's graph), the launch rule of include/poi_hip.h on top of it, and
the scoring in the literal (n_item + 1, 4, depth, rows) form and in the factorised form the kernel uses.

Tables P = {"xu": (n_user, D), "wl": (n_item, D), "pb": (n_node, D)}; tree T = {"routes": (n_item + 1, 4, depth), "lrs": same,
"probs": (n_item + 1, 4)} with the pad row n_item.  A user's data: targets (L,), contexts = list of L integer arrays (ids >= n_item are
the reference's padding: they add the zero row wl_m)."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def context_sum(wl, ctx):
    c = np.zeros(wl.shape[1])
    for k in ctx:
        if 0 <= k < len(wl):
            c += wl[k]
    return c


def forward_terms(P, T, u, targets, contexts):
    """The per-position quantities of POI2Vec.py:140-151 for one user -> dict (cl, ind, z, sig, prod, S, paths, logp, lse)."""
    xu, wl, pb = P["xu"], P["wl"], P["pb"]
    targets = np.asarray(targets, np.int64)
    L = len(targets)
    s = wl @ xu[u]
    m = s.max()
    lse = m + np.log(np.exp(s - m).sum())
    cl = np.stack([context_sum(wl, c) for c in contexts]) if L else np.zeros((0, wl.shape[1]))
    ind = np.ceil(np.abs(cl.mean(axis=1)))                                            # :148 T.ceil(abs(T.mean(cl, axis=3)))
    routes, lrs, probs = T["routes"][targets], T["lrs"][targets].astype(np.float64), T["probs"][targets].astype(np.float64)
    z = np.einsum("irdk,ik->ird", pb[routes], cl)
    sig = _sig(z * lrs)
    br = sig * ind[:, None, None]
    prod = br.prod(axis=2)
    S = (prod * probs).sum(axis=1)
    paths = np.floor(1 - S) + S                                                       # :152-153
    return dict(s=s, lse=lse, cl=cl, ind=ind, z=z, sig=sig, br=br, prod=prod, S=S, paths=paths, routes=routes, lrs=lrs, probs=probs)


def user_terms(P, T, u, targets, contexts, alpha, lam, len_max):
    """One user at the values P: (loss upq, {"wl": dense (n_item, D) delta, "xu": (D,) delta of row u, "pb": {node: delta}}).  The pb deltas
    are the collapsed ones: per occurrence (i, r, d) new = old - alpha grad of that occurrence, assigned in the flattened order of the bidx
    padded to len_max (POI2Vec.py:163-165, 175: set_subtensor on pb[bidx]; numpy's last-wins) - positions i >= L route through routes[0]
    and write the old value back, so a node on them is absent from the dict (a padding write is not a touch)."""
    xu, wl, pb = P["xu"], P["wl"], P["pb"]
    targets = np.asarray(targets, np.int64)
    L, n_item = len(targets), len(wl)
    F = forward_terms(P, T, u, targets, contexts)
    with np.errstate(all="ignore"):
        loss = -np.sum(F["s"][targets] - F["lse"] + np.log(F["paths"])) / L
    sm = np.exp(F["s"] - F["lse"])
    cnt = np.bincount(targets, minlength=n_item).astype(np.float64)
    G = sm - cnt / L
    g_wl = np.outer(G, xu[u]) + lam * wl
    g_xu = G @ wl + lam * xu[u]
    dS = -(1.0 / L) / F["paths"]                                                      # d upq / d S_i (floor carries no gradient)
    # d S_i / d z_ird = probs_ir prod_ir (1 - sig_ird) lr_ird  (prod / br * d br / d z; the ceil factor is a constant)
    others = np.empty_like(F["br"])
    depth = F["br"].shape[2]
    for d in range(depth):
        others[:, :, d] = np.prod(np.delete(F["br"], d, axis=2), axis=2)
    gz = dS[:, None, None] * F["probs"][:, :, None] * others * (F["sig"] * (1 - F["sig"]) * F["ind"][:, None, None]) * F["lrs"]
    gc = np.einsum("ird,irdk->ik", gz, pb[F["routes"]])
    for i, c in enumerate(contexts):
        for k in c:
            if 0 <= k < n_item:
                g_wl[k] += gc[i]
    new_pb = {}
    for i in range(L):
        for r in range(4):
            for d in range(depth):
                new_pb[int(F["routes"][i, r, d])] = -alpha * gz[i, r, d] * F["cl"][i]
    if L < len_max:
        for n in np.unique(T["routes"][0]):
            new_pb.pop(int(n), None)
    return loss, dict(wl=-alpha * g_wl, xu=-alpha * g_xu, pb=new_pb)


def step(P, T, u, targets, contexts, alpha, lam, len_max):
    """Poi2vec.train(u) (POI2Vec.py:127-181): (new tables, upq)."""
    loss, dl = user_terms(P, T, u, targets, contexts, alpha, lam, len_max)
    Q = {k: v.copy() for k, v in P.items()}
    Q["wl"] += dl["wl"]
    Q["xu"][u] += dl["xu"]
    for n, v in dl["pb"].items():
        Q["pb"][n] += v
    return Q, loss


def batch_step(P, T, users, data, alpha, lam, len_max, cap=1.0, absmass=False):
    """A launch under the snapshot rule with the cap (include/poi_hip.h): every user at the launch-entry values; wl is touched by every
    accepted user, an xu row by its user(s), a pb row by the users whose collapsed write on it comes from a real position; a row touched
    by k users moves by min(k, cap) / k times their summed deltas.  data[u] = (targets, contexts).  A user with an id out of range,
    L = 0, a target outside [0, n_item) or a non-finite loss is rejected: NaN loss, moves nothing."""
    sums = {k: np.zeros_like(v) for k, v in P.items()}
    mass = {k: np.zeros_like(v) for k, v in P.items()}
    cnt = {k: np.zeros(len(v), np.int64) for k, v in P.items()}
    losses = np.full(len(users), np.nan)
    n_user, n_item = len(P["xu"]), len(P["wl"])
    for t, u in enumerate(users):
        u = int(u)
        if not 0 <= u < n_user:
            continue
        targets, contexts = data[u]
        targets = np.asarray(targets, np.int64)
        if len(targets) == 0 or targets.min() < 0 or targets.max() >= n_item:
            continue
        loss, dl = user_terms(P, T, u, targets, contexts, alpha, lam, len_max)
        if not np.isfinite(loss):
            continue
        losses[t] = loss
        sums["wl"] += dl["wl"]; mass["wl"] += np.abs(dl["wl"]); cnt["wl"] += 1
        sums["xu"][u] += dl["xu"]; mass["xu"][u] += np.abs(dl["xu"]); cnt["xu"][u] += 1
        for n, v in dl["pb"].items():
            sums["pb"][n] += v; mass["pb"][n] += np.abs(v); cnt["pb"][n] += 1
    Q, M = {}, {}
    for k in P:
        k_ = cnt[k].astype(np.float64)
        f = np.where(k_ > 0, np.minimum(k_, cap) / np.maximum(k_, 1.0), 0.0)[:, None]
        Q[k] = P[k] + f * sums[k]
        M[k] = f * mass[k]
    return (Q, losses, M) if absmass else (Q, losses)


def l2(P, lam):
    """POI2Vec.py:116-122."""
    return 0.5 * lam * sum(float((P[k] ** 2).sum()) for k in ("xu", "pb", "wl"))


# ---- scoring (POI2Vec.py:91-109) -----------------------------------------------------------------------------------------------------
def plu_matrix(P, users, softmax_axis="reference"):
    """(n_batch, n_item): softmax of xu[users] . wl^T over the USERS of the batch ("reference": the 2-D call of softmax(), axis 0, :92 and
    :183-186) or over the POIs ("items")."""
    s = P["xu"][np.asarray(users, np.int64)] @ P["wl"].T
    ax = 0 if softmax_axis == "reference" else 1
    e = np.exp(s - s.max(axis=ax, keepdims=True))
    return e / e.sum(axis=ax, keepdims=True)


def scores_literal(P, T, users, cl, softmax_axis="reference"):
    """The reference's own form: cl (n_batch, length, D) context sums; pb[routes] (n_item + 1, 4, depth, D) times cl -> rows ordered
    (user, position): (n_batch * length, n_item)."""
    plu = plu_matrix(P, users, softmax_axis)
    nb, length, D = cl.shape
    pb = P["pb"][T["routes"]]
    lrs = T["lrs"].astype(np.float64)[:, :, :, None, None]
    pr_bc = np.einsum("jrdk,btk->jrdtb", pb, cl)
    br = _sig(pr_bc * lrs) * np.ceil(np.abs(pr_bc))
    path = br.prod(axis=2) * T["probs"].astype(np.float64)[:, :, None, None]
    paths = path.sum(axis=1)
    paths = np.floor(1 - paths) + paths
    p = paths[:-1].T * plu.reshape(nb, 1, -1)
    return p.reshape(nb * length, -1)


def route_table(T):
    """The distinct routes of the tree: (node ids (n_route, depth), lrs (n_route, depth), index (n_item + 1, 4) of each POI's routes)."""
    flat = np.concatenate([T["routes"].reshape(-1, T["routes"].shape[2]), T["lrs"].reshape(-1, T["lrs"].shape[2]).astype(np.int32)], 1)
    uniq, inv = np.unique(flat, axis=0, return_inverse=True)
    depth = T["routes"].shape[2]
    return uniq[:, :depth], uniq[:, depth:], inv.reshape(T["routes"].shape[:2])


def scores_factorised(P, T, users, cl, softmax_axis="reference", return_z=False):
    """The kernel's form: the n_node products per row once, the product along each distinct route, 4 gathers per POI."""
    plu = plu_matrix(P, users, softmax_axis)
    nb, length, D = cl.shape
    rows = cl.reshape(nb * length, D)
    z = rows @ P["pb"].T                                                              # (rows, n_node)
    rn, rl, ridx = route_table(T)
    zr = z[:, rn]                                                                     # (rows, n_route, depth)
    f = _sig(zr * rl[None].astype(np.float64)) * np.ceil(np.abs(zr))
    rp = f.prod(axis=2)                                                               # (rows, n_route)
    S = (rp[:, ridx[:-1]] * T["probs"].astype(np.float64)[None, :-1]).sum(axis=2)     # (rows, n_item)
    paths = np.floor(1 - S) + S
    out = paths * np.repeat(plu, length, axis=0)
    return (out, z, S) if return_z else out


def topk_desc(scores, k):
    """Descending score, then ascending id."""
    s = np.asarray(scores)
    order = np.lexsort((np.arange(s.shape[1])[None, :].repeat(len(s), 0), -s), axis=1)
    return order[:, :k].astype(np.int32)
