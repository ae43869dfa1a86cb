"""numpy oracle of the filtered recommendation (poi_filter_build, poi_score_topk_filtered, poi_topk_filtered_scores ->
models.compute_sub_topk_filtered): pass bits from predicates, and the definition of include/poi_hip.h applied to a given float32 score
matrix and a candidate mask - the tie rule, the fill, the selectable rule and the signed zeros.  Radius masks and float64 scores come
from tests/near_oracle.py.  Never the code under test: host numpy only, written with loops where the product packs with shifts."""
import numpy as np

K_MAX = 32


def pass_mask(cat, flags, n_cat, predicates):
    """((P, n_item) bool, strays): predicate q = dict(categories=[..], need=, any=, forbid=), every key optional.
    pass = (no list or cat in list) and (flags & need) == need and (any == 0 or flags & any) and not (flags & forbid).
    A NULL flags reads as zeros.  strays = the POIs whose category lies outside [0, n_cat) (they pass no predicate that has a list),
    counted once per POI when a category array is given."""
    n_item = len(cat) if cat is not None else len(flags)
    f = np.zeros(n_item, np.uint64) if flags is None else np.asarray(flags).astype(np.uint64)
    out = np.zeros((len(predicates), n_item), bool)
    stray = np.zeros(n_item, bool) if cat is None else (np.asarray(cat) < 0) | (np.asarray(cat) >= n_cat)
    for q, d in enumerate(predicates):
        need, any_, forbid = (np.uint64(d.get(key, 0)) for key in ("need", "any", "forbid"))
        ok = ((f & need) == need) & ((f & forbid) == 0)
        if any_:
            ok &= (f & any_) != 0
        cats = list(d.get("categories") or ())
        if cats:
            assert cat is not None, "a category list needs categories"
            ok &= np.isin(np.asarray(cat), cats) & ~stray
        out[q] = ok
    return out, int(stray.sum())


def bits(mask, ldw=None):
    """(P, ldw) uint32: POI j is bit j & 31 of word j >> 5; everything at j >= n_item is 0."""
    mask = np.atleast_2d(np.asarray(mask, bool))
    P, N = mask.shape
    W = (N + 31) // 32
    ldw = W if ldw is None else ldw
    out = np.zeros((P, ldw), np.uint32)
    for q in range(P):
        for j in np.nonzero(mask[q])[0]:
            out[q, j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    return out


def unpack(words, n_item):
    """The inverse of bits() over the first n_item positions: (P, n_item) bool."""
    words = np.atleast_2d(words)
    j = np.arange(n_item)
    return ((words[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, (np.concatenate([np.asarray(l, np.int64) for l in lists]).astype(np.int32) if off[-1] else np.zeros(0, np.int32))


def candidate_masks(pmask, pred, n, ex_off=None, ex=None, anchor=None, radius_mask=None):
    """((n, n_item) bool C(r), bad (n) bool).  pmask (P, n_item): the predicates' pass masks; pred (n) or None (predicate 0);
    radius_mask (n, n_item) or None: near_oracle.candidate_mask WITHOUT lists (it lets the anchor in; here the anchor must pass too,
    which the AND with the pass mask says).  A row is bad - an empty C(r) - when its predicate index leaves [0, P), its anchor leaves
    [-1, n_item) or its list is not strictly ascending inside [0, n_item)."""
    P, N = pmask.shape
    pred = np.zeros(n, np.int64) if pred is None else np.asarray(pred, np.int64)
    mask, bad = np.zeros((n, N), bool), np.zeros(n, bool)
    for r in range(n):
        lst = np.zeros(0, np.int64) if ex_off is None else np.asarray(ex[ex_off[r]:ex_off[r + 1]], np.int64)
        if ex_off is not None and (ex_off[r] < 0 or ex_off[r + 1] < ex_off[r]):
            bad[r] = True
        if not 0 <= pred[r] < P or (anchor is not None and not -1 <= anchor[r] < N):
            bad[r] = True
        if len(lst) and (lst.min() < 0 or lst.max() >= N or np.any(np.diff(lst) <= 0)):
            bad[r] = True
        if bad[r]:
            continue
        mask[r] = pmask[pred[r]]
        if radius_mask is not None:
            mask[r] &= radius_mask[r]
        mask[r, lst] = False
    return mask, bad


def topk(sc, mask, k):
    """The definition on float32 scores sc (n, >= n_item) and C(r) = mask: (ids (n, k) int32 with -1 fill, scores float32 with -inf
    fill, counts = |C(r)|).  Selectable: neither NaN nor -inf (+inf is).  -0.0 and +0.0 are one score, written +0.0.  Higher score
    first, then the lower id."""
    sc = np.asarray(sc, np.float32)
    n, N = mask.shape
    ids, val = np.full((n, k), -1, np.int32), np.full((n, k), -np.inf, np.float32)
    for r in range(n):
        s = sc[r, :N].copy()
        s[s == 0] = 0.0                              # one zero
        cand = np.nonzero(mask[r] & ~np.isnan(s) & ~np.isneginf(s))[0]
        order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))][:k]
        ids[r, :len(order)] = order
        val[r, :len(order)] = s[order]
    return ids, val, mask.sum(axis=1).astype(np.int32)
