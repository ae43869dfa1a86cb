"""numpy float64 oracle of the label recommendation (include/poi_hip.h: poi_score_labels, poi_score_topk_labels, poi_labels_scores).
The definition with its integer q: per row M = the maximum of the non-NaN scores of ALL POIs, per candidate q = rint(exp(s - M) 2^36)
as uint64, per bucket (label 0 .. n_label - 1, bucket n_label = the unlabelled POIs) the uint64 sum of q, the candidate that wins under
"higher score, then lower id", and the number of candidates; both orders; the dense and the top-K form; and the rule that says on
which rows a float32 implementation must reproduce the float64 label order ("clear" rows).  Pure numpy, no GPU."""
import numpy as np

Q_BITS = 36
Q_ONE = float(1 << Q_BITS)
NEG_INF = -np.inf


def f64(a):
    return np.asarray(a, dtype=np.float64)


def one_zero(sc):
    """The scores as ranked: -0.0 is +0.0 (dtype kept)."""
    sc = np.array(sc, copy=True)
    sc[sc == 0] = 0
    return sc


def row_max(sc):
    """M (n) in the dtype of sc: the maximum over the non-NaN scores of a row, -inf for a row without any."""
    sc = one_zero(np.atleast_2d(sc))
    return np.where(np.isnan(sc), -np.inf, sc).max(axis=1, initial=-np.inf).astype(sc.dtype)


def q_terms(sc, M):
    """q (n, n_item) uint64 of every POI with a selectable score (0 elsewhere, and on rows whose M is not finite)."""
    sc = f64(one_zero(np.atleast_2d(sc)))
    M = f64(M)
    fin = np.isfinite(M)
    ok = fin[:, None] & ~np.isnan(sc) & (sc > -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(np.where(ok, sc - np.where(fin, M, 0.0)[:, None], -np.inf))
    return np.rint(e * Q_ONE).astype(np.uint64), ok


def buckets(labels, n_label):
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 0) & (lab < n_label), lab, n_label)


def dense(sc, mask, labels, n_label):
    """dict(mass (n, n_label + 1) uint64, best_id int32 (-1: none), best_score (dtype of sc; -inf: none), count int32, M (n), total
    (n) uint64) of score rows sc (n, n_item) under the candidate masks mask (n, n_item) bool (None: every POI)."""
    sc = one_zero(np.atleast_2d(sc))
    n, N = sc.shape
    mask = np.ones((n, N), bool) if mask is None else np.asarray(mask, bool)
    M = row_max(sc)
    q, ok = q_terms(sc, M)
    cand = ok & mask
    b = buckets(labels, n_label)
    L1 = n_label + 1
    mass = np.zeros((n, L1), np.uint64)
    count = np.zeros((n, L1), np.int32)
    best_id = np.full((n, L1), -1, np.int32)
    best_score = np.full((n, L1), -np.inf, sc.dtype)
    for r in range(n):
        j = np.nonzero(cand[r])[0]
        if not len(j):
            continue
        np.add.at(mass[r], b[j], q[r, j])
        np.add.at(count[r], b[j], 1)
        order = j[np.lexsort((j, -f64(sc[r, j])))]                     # by better(): higher score, then lower id
        first = np.unique(b[order], return_index=True)
        best_id[r, first[0]] = order[first[1]]
        best_score[r, first[0]] = sc[r, order[first[1]]]
    return dict(mass=mass, best_id=best_id, best_score=best_score, count=count, M=M, total=mass.sum(axis=1, dtype=np.uint64))


def log_share(mass, total):
    """log(mass) - log(total) in float64, -inf where the mass is 0."""
    mass, total = f64(mass), f64(total)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mass > 0, np.log(np.where(mass > 0, mass, 1.0)) - np.log(np.where(total > 0, total, 1.0)), -np.inf)


def lognorm(D):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D["total"] > 0, f64(D["M"]) + np.log(f64(D["total"]) / Q_ONE), -np.inf)


def topk(D, by, k):
    """The top-K form of a dense result: dict(label (n, k) int32 (-1 fill), logp (n, k) float64 (-inf fill), best_id, best_score,
    n_listed (n), rest_logp (n)).  by "mass": higher mass, then lower label; "max": the label's best POI under better()."""
    n, L1 = D["mass"].shape
    L = L1 - 1
    label = np.full((n, k), -1, np.int32)
    logp = np.full((n, k), -np.inf)
    best_id = np.full((n, k), -1, np.int32)
    best_score = np.full((n, k), -np.inf, D["best_score"].dtype)
    n_listed = np.zeros(n, np.int32)
    for r in range(n):
        ls = np.nonzero(D["count"][r, :L] > 0)[0]
        if by == "mass":
            ls = np.array(sorted(ls, key=lambda l: (-int(D["mass"][r, l]), l)), np.int64)      # (exact integers: no float order)
        else:
            ls = ls[np.lexsort((D["best_id"][r, ls], -f64(D["best_score"][r, ls])))]
        ls = ls[:k]
        m = len(ls)
        n_listed[r] = m
        label[r, :m] = ls
        logp[r, :m] = log_share(D["mass"][r, ls], D["total"][r])
        best_id[r, :m] = D["best_id"][r, ls]
        best_score[r, :m] = D["best_score"][r, ls]
    return dict(label=label, logp=logp, best_id=best_id, best_score=best_score, n_listed=n_listed,
                rest_logp=log_share(D["mass"][:, L], D["total"]))


def clear_rows(D, sc, by, k, margin=1e-5):
    """(n) bool: every adjacent pair of the top k + 1 labels' log-masses (by "mass") or best scores (by "max") differs by at least
    margin max(1, max |score|) - on such a row an implementation within that tolerance must list the same labels in the same order."""
    fin = np.abs(np.where(np.isfinite(sc), sc, 0.0))
    tol = margin * max(1.0, float(fin.max(initial=0.0)))
    T = topk(D, by, k + 1)
    v = T["logp"] if by == "mass" else f64(T["best_score"])
    ok = np.ones(len(v), bool)
    for r in range(len(v)):
        m = int(T["n_listed"][r])
        x = v[r, :m]
        x = x[np.isfinite(x)] if by == "mass" else x
        if by == "mass" and len(x) < m:                 # labels without mass tie at -inf: clear only if they lie behind the list
            ok[r] = len(x) >= min(m, k)
        ok[r] &= bool(np.all(x[:-1] - x[1:] >= tol))
    return ok


def clear_rows_tight(D, by, k):
    """(n) bool, for an implementation that reads the SAME float32 rows as the oracle: by "max" every row is clear (the order is exact);
    by "mass" the two exp routines may differ by one unit of q per term, so two labels are told apart for certain when their masses
    differ by more than the sum of their counts - required of every adjacent pair of the top k + 1."""
    n = len(D["mass"])
    ok = np.ones(n, bool)
    if by == "mass":
        T = topk(D, by, k + 1)
        for r in range(n):
            ls = T["label"][r, :int(T["n_listed"][r])]
            ms = [int(D["mass"][r, l]) for l in ls]
            cs = [int(D["count"][r, l]) for l in ls]
            ok[r] = all(ms[i] - ms[i + 1] > cs[i] + cs[i + 1] for i in range(len(ls) - 1))
    return ok
