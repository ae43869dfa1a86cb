"""numpy oracle of the capped recommendation (poi_labels_build, poi_score_topk_capped, poi_topk_capped_scores ->
models.compute_sub_topk_capped): the definition of include/poi_hip.h applied to a given score matrix, a candidate mask and a
labelling - in its greedy form and in its counting form -, the fill table, the pairwise merge with re-capping that the kernels use and
the shortcut they do not, and the qualifying rule of the independence test.  Candidate masks come from tests/filter_oracle.py.  Never
the code under test: host numpy only, written with loops."""
import numpy as np

K_MAX = 32
PER_MAX = 32


def ranked(sc_row, mask_row):
    """The selectable candidates of a row by better(): descending score (one zero), ascending id -> (ids, scores float32)."""
    s = np.asarray(sc_row, np.float32).copy()
    s[s == 0] = 0.0
    cand = np.nonzero(np.asarray(mask_row, bool) & ~np.isnan(s) & ~np.isneginf(s))[0]
    order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))]
    return order, s[order]


def greedy(order, labels, per, k):
    """Walk `order`; take j unless labels[j] >= 0 and `per` taken entries carry labels[j]; stop at k -> (positions taken, examined):
    examined = the position in `order` of the k-th taken entry + 1 (len(order) if the list does not fill)."""
    taken, have = [], {}
    for pos, j in enumerate(order):
        l = int(labels[j])
        if l >= 0:
            if have.get(l, 0) >= per:
                continue
            have[l] = have.get(l, 0) + 1
        taken.append(pos)
        if len(taken) == k:
            return taken, pos + 1
    return taken, len(order)


def counting(order, labels, per, k):
    """The non-sequential form: j is kept iff fewer than `per` candidates of its label precede it; the first k kept."""
    lab = np.asarray(labels)[order]
    keep = []
    for pos in range(len(order)):
        if lab[pos] < 0 or int((lab[:pos] == lab[pos]).sum()) < per:
            keep.append(pos)
    return keep[:k]


def topk(sc, mask, labels, per, k, form=greedy):
    """(ids (n, k) int32 with -1 fill, scores float32 with -inf fill, labels int32 with -1 fill, counts = |C(r)|)."""
    sc = np.asarray(sc, np.float32)
    n, N = mask.shape
    labels = np.asarray(labels)
    ids, val = np.full((n, k), -1, np.int32), np.full((n, k), -np.inf, np.float32)
    lab = np.full((n, k), -1, np.int32)
    for r in range(n):
        order, s = ranked(sc[r, :N], mask[r])
        got = form(order, labels, per, k)
        pos = got[0] if form is greedy else got
        ids[r, :len(pos)] = order[pos]
        val[r, :len(pos)] = s[pos]
        lab[r, :len(pos)] = labels[order[pos]]
    return ids, val, lab, mask.sum(axis=1).astype(np.int32)


def fill_table(labels, n_label, pmask=None):
    """(fill (P, 33), counts (n_label), strays): fill[q][m] = #(unlabelled POIs passing q) + sum over labels of min(m, #passing POIs of
    the label).  pmask None: one row, every POI passes.  A label >= n_label is a stray: counted once per POI, entered as unlabelled.
    counts: the POIs of every label in [0, n_label), whatever they pass."""
    labels = np.asarray(labels, np.int64)
    pmask = np.ones((1, len(labels)), bool) if pmask is None else np.atleast_2d(np.asarray(pmask, bool))
    stray = labels >= n_label
    grouped = (labels >= 0) & ~stray
    fill = np.zeros((len(pmask), PER_MAX + 1), np.int32)
    for q, row in enumerate(pmask):
        h = np.zeros(n_label, np.int64)
        for j in np.nonzero(row & grouped)[0]:
            h[labels[j]] += 1
        unl = int((row & ~grouped).sum())
        for m in range(PER_MAX + 1):
            fill[q, m] = unl + int(np.minimum(h, m).sum())
    counts = np.zeros(n_label, np.int32)
    for j in np.nonzero(grouped)[0]:
        counts[labels[j]] += 1
    return fill, counts, int(stray.sum())


# ---- lists of (score, id) pairs: what the kernels merge ------------------------------------------------------------------------------
def sort_entries(entries):
    return sorted(entries, key=lambda e: (-float(e[0]), e[1]))


def recap(entries, labels, per, k):
    """Sort, keep an entry iff fewer than `per` same-label entries precede it, cut to k."""
    out, seen = [], {}
    for s, j in sort_entries(entries):
        l = int(labels[j])
        if l >= 0:
            if seen.get(l, 0) >= per:
                seen[l] += 1
                continue
            seen[l] = seen.get(l, 0) + 1
        out.append((s, j))
    return out[:k]


def merge_pairwise(lists, labels, per, k):
    """Fold the partial lists in order, two at a time, re-capping after EVERY merge: the rule the kernels use."""
    acc = recap(lists[0], labels, per, k)
    for nxt in lists[1:]:
        acc = recap(acc + list(nxt), labels, per, k)
    return acc


def merge_best_then_cap(lists, labels, per, k, depth=None):
    """The shortcut the kernels do NOT take: the plain best `depth` (default 2 k) of the union of all lists, capped once."""
    union = sort_entries([e for l in lists for e in l])[:2 * k if depth is None else depth]
    return recap(union, labels, per, k)


def qualifying(osc, mask, labels, per, k, margin=1e-6):
    """Rows on which float32 rounding cannot change the capped list: every adjacent gap among the candidates the greedy pass examines,
    down to and including the first one behind the k-th accepted entry, is at least margin * max|score| (near_oracle.qualifying's
    margin, extended to the depth the cap looks at) -> (ok (n) bool, depth examined (n))."""
    tol = margin * np.abs(osc[np.isfinite(osc)]).max()
    n = mask.shape[0]
    ok, depth = np.zeros(n, bool), np.zeros(n, np.int64)
    for r in range(n):
        cand = np.nonzero(mask[r])[0]
        order = cand[np.lexsort((cand, -osc[r, cand]))]
        _, seen = greedy(order, labels, per, k)
        d = min(seen + 1, len(order))
        depth[r] = d
        ok[r] = d < 2 or bool(np.all(-np.diff(osc[r, order[:d]]) >= tol))
    return ok, depth
