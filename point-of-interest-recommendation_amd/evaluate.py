"""Evaluator in the shape of public/Valuate.py: AUC from model.compute_sub_auc_preference, top-K from
the fused device kernel (model.compute_sub_topk) instead of (n, N) score matrices + per-row numpy
argpartition, then hit / recall / precision / F1 / MAP / NDCG @ at_nums (Valuate.py:23-88,149-172),
vectorised over users."""
from __future__ import annotations

import numpy as np


class GlobalBest:
    """Best-so-far bookkeeping (public/Global_Best.py:21-82, without the printing)."""

    def __init__(self, at_nums):
        self.at_nums = list(at_nums)
        z = lambda: np.zeros(len(at_nums))
        self.best_auc, self.best_epoch_auc = 0.0, 0
        for n in ("recall", "precis", "f1scor", "map", "ndcg"):
            setattr(self, "best_" + n, z())
            setattr(self, "best_epoch_" + n, np.zeros(len(at_nums), int))


def rank_metrics(all_ranks, tes_buys_masks, tes_masks, at_nums):
    """Valuate.py:149-172 on an (U, Kmax) rank matrix.  Returns {k: dict(hits, recall, precision, f1, map, ndcg)}."""
    ranks = np.asarray(all_ranks)
    tes = np.asarray(tes_buys_masks)
    msk = np.asarray(tes_masks).astype(bool)
    n_test = msk.sum(axis=1)                                       # len(test_lst) per user
    denom = float(msk.sum())
    out = {}
    for k in at_nums:
        rec = ranks[:, :k]
        # zero_one[u, r] = 1 if rec[u, r] is one of the user's valid test items (fun_hit_zero_one)
        zo = ((rec[:, :, None] == tes[:, None, :]) & msk[:, None, :]).any(axis=2).astype(np.int64)
        hits = float(zo.sum())
        recall = hits / denom
        precis = hits / (k * len(zo))
        f1 = 2.0 * recall * precis / (recall + precis) if recall + precis > 0 else 0.0
        cum = zo.cumsum(axis=1) * zo                               # fun_evaluate_map
        ap = (cum / np.arange(1, k + 1)[None, :]).sum(axis=1) / np.maximum(n_test, 1)
        disc = 1.0 / np.log2(np.arange(k) + 2.0)                   # fun_evaluate_ndcg
        dcg = (zo * disc[None, :]).sum(axis=1)
        ideal = np.array([disc[:min(int(t), k)].sum() for t in n_test])
        ndcg = np.where(zo.sum(axis=1) > 0, dcg / np.maximum(ideal, 1e-300), 0.0)
        out[k] = dict(hits=hits, recall=recall, precision=precis, f1=f1, map=float(ap.mean()), ndcg=float(ndcg.mean()))
    return out


def coalesce_ranges(starts_ends, target=65536):
    """Merge consecutive contiguous id ranges into calls of up to `target` users.  The reference evaluates in
    batch_size_test users per call (Params.compute_start_end); the metrics are sums over users, so the grouping is
    free - and the two-stage scoring path is at its best with as many users per call as there are (call sizes;
    the cap bounds the per-call survivor lists: 32 KB per user)."""
    out, cur = [], None
    for se in starts_ends:
        se = np.asarray(se)
        contiguous = len(se) > 0 and np.all(np.diff(se) == 1)
        if cur is not None and contiguous and len(cur) and cur[-1] + 1 == se[0] and len(cur) + len(se) <= target:
            cur = np.concatenate((cur, se))
        else:
            if cur is not None:
                out.append(cur)
            cur = se
    if cur is not None:
        out.append(cur)
    return out


def device_rank_metrics(model, starts_ends_tes, at_nums, within_km=None, exclude=None):
    """Fused top-K + metric accumulation on the device: only (len(at_nums), 3) doubles reach the host.
    within_km / exclude (model.compute_sub_topk_near; cut-offs <= 32): rank over the POIs within that radius of the user's last train
    POI, minus the exclusion lists - the restricted-candidate protocol of the FPMC-LR paper.  A row with fewer candidates than the
    cut-off carries -1 ids, which poi_rank_metrics counts as misses (an id equals no test POI)."""
    import ctypes
    import torch
    at_nums = list(at_nums)
    if not at_nums or len(at_nums) > 8 or any(b <= a for a, b in zip(at_nums, at_nums[1:])) or at_nums[0] <= 0 or at_nums[-1] > 64:
        raise ValueError("at_nums must be 1..8 strictly ascending cut-offs <= 64 (got %r)" % (at_nums,))
    kmax = at_nums[-1]
    acc = torch.zeros((len(at_nums), 3), dtype=torch.float64, device=model.device)
    at = torch.as_tensor(np.asarray(at_nums, np.int32)).to(model.device)
    for se in coalesce_ranges(starts_ends_tes):
        ids, lo = model._ids(se)
        if within_km is None and exclude is None:
            idx = model.compute_sub_topk(se, kmax)
        else:
            idx = model.compute_sub_topk_near(se, kmax, within_km=within_km, exclude=exclude)
        tp, tm = model._rows(model.tes_buys_masks, ids, lo), model._rows(model.tes_masks, ids, lo)
        model.ctx.check(model.lib.poi_rank_metrics(model.ctx.handle, idx.data_ptr(), idx.shape[0], kmax, tp.data_ptr(), tm.data_ptr(),
                                                   tm.shape[1], at.data_ptr(), len(at_nums), acc.data_ptr(), model._stream()))
    a = acc.cpu().numpy()
    n_user = model.n_user
    denom = float(model.tes_masks.sum().item())
    out = {}
    for i, k in enumerate(at_nums):
        hits = float(a[i, 0]); rec = hits / denom; pre = hits / (k * n_user)
        out[k] = dict(hits=hits, recall=rec, precision=pre, f1=2.0 * rec * pre / (rec + pre) if rec + pre > 0 else 0.0,
                      map=float(a[i, 1]) / n_user, ndcg=float(a[i, 2]) / n_user)
    return out


def rank_summary(ranks, counts, at_nums, n_user=None):
    """The formulas of full_rank_metrics on host arrays: ranks (n, len_t) with -1 = not ranked, counts (n) ranked POIs per row.
    hits / recall / ndcg agree with rank_metrics on a list built from the same ranks (a target at rank < k is a hit at position rank;
    distinct valid targets of a row have distinct ranks)."""
    ranks = np.asarray(ranks, np.int64)
    counts = np.asarray(counts, np.int64)
    ok = ranks >= 0
    denom = float(ok.sum())
    r = ranks[ok].astype(np.float64)
    c = np.broadcast_to(counts[:, None], ranks.shape)[ok].astype(np.float64)
    n_user = len(ranks) if n_user is None else n_user
    n_test = ok.sum(axis=1)
    out = dict(n=denom, mrr=float((1.0 / (r + 1.0)).sum() / denom) if denom else 0.0, mean_rank=float(r.mean()) if denom else 0.0,
               median_rank=float(np.sort(r)[(len(r) - 1) // 2]) if denom else 0.0,
               auc_full=float(np.where(c > 1, 1.0 - r / np.maximum(c - 1.0, 1.0), 1.0).sum() / denom) if denom else 0.0, at={})
    for k in at_nums:
        hit = ok & (ranks < k)
        disc = np.where(hit, 1.0 / np.log2(np.maximum(ranks, 0) + 2.0), 0.0)
        ideal = np.array([(1.0 / np.log2(np.arange(min(int(t), k)) + 2.0)).sum() for t in n_test])
        ndcg = np.where(hit.any(axis=1), disc.sum(axis=1) / np.maximum(ideal, 1e-300), 0.0)
        hits = float(hit.sum())
        out["at"][k] = dict(hits=hits, recall=hits / denom if denom else 0.0, ndcg=float(ndcg.sum() / n_user))
    return out


def full_rank_metrics(model, starts_ends_tes, at_nums, exclude=None):
    """Metrics from the EXACT rank of every held-out POI among all POIs (model.compute_sub_target_rank): independent of the negative
    sampler and of any list length.  Returns dict(n, mrr, mean_rank, median_rank (the lower median), auc_full = mean of
    1 - rank / (count - 1) - the share of the other ranked POIs that score below the target -, at = {k: dict(hits, recall, ndcg)}) for
    any ascending cut-offs 1 <= k <= n_item; recall / ndcg follow rank_metrics' definitions.  exclude as compute_sub_target_rank (a
    target that is excluded is not ranked and leaves every mean).  The reductions are torch ops on the device; scalars reach the host."""
    batches = (model.compute_sub_target_rank(se, exclude=exclude, return_counts=True) for se in coalesce_ranges(starts_ends_tes))
    return _metrics_of_ranks(model, batches, at_nums, model.tes_masks.shape[1], model.n_user)


def candidate_recall(model, starts_ends_tes, ks, exclude="train"):
    """Recall of the retrieval stage: the share of the held-out POIs (tes_buys_masks under tes_masks) that lie inside the top-k
    candidates of model.compute_sub_candidates, for every k in ks (strictly ascending, 1 <= k <= min(4096, n_item)).  All cut-offs come
    from ONE call at max(ks): the list is sorted, so the top-k is its first k columns.  exclude as compute_sub_candidates; a held-out POI
    that is excluded (or lies outside [0, n_item)) is not a candidate and leaves the mean, as in full_rank_metrics - whose recall at
    the same cut-offs this equals.  Returns {k: recall}; the reductions are torch ops on the device."""
    import torch
    ks = [int(k) for k in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] <= 0:
        raise ValueError("ks must be strictly ascending cut-offs >= 1 (got %r)" % (ks,))
    N = model.n_item
    hits = torch.zeros(len(ks), dtype=torch.float64, device=model.device)
    total = torch.zeros((), dtype=torch.float64, device=model.device)
    for se in coalesce_ranges(starts_ends_tes):
        idx = model.compute_sub_candidates(se, ks[-1], exclude=exclude)
        ids, lo = model._ids(se)
        n = ids.numel()
        tgt = model._rows(model.tes_buys_masks, ids, lo).long()
        ok = (model._rows(model.tes_masks, ids, lo) != 0) & (tgt >= 0) & (tgt < N)
        eo, ex = model._near_exclusion(exclude, n, None, ids, lo, kinds=("train",))
        if eo is not None and n:                                     # a target on its row's list: sorted keys row * n_item + id
            eo = eo.long()
            rows = torch.repeat_interleave(torch.arange(n, device=model.device), eo[1:] - eo[:-1])
            keys = rows * N + ex[int(eo[0]):int(eo[-1])].long()
            want = torch.arange(n, device=model.device)[:, None] * N + tgt.clamp(0, N - 1)
            at = torch.searchsorted(keys, want.reshape(-1)).clamp(max=max(keys.numel() - 1, 0)).reshape(want.shape)
            ok &= ~((keys[at] == want) if keys.numel() else torch.zeros_like(ok))
        total += ok.sum()
        for o in range(0, n, 2048):                                  # (rows, targets, k) comparisons, 2048 rows at a time
            eq = idx[o:o + 2048, None, :] == tgt[o:o + 2048, :, None].int()
            found = eq.any(2) & ok[o:o + 2048]
            pos = eq.int().argmax(2)
            for i, k in enumerate(ks):
                hits[i] += (found & (pos < k)).sum()
    h, t = hits.cpu().numpy(), float(total.item())
    return {k: (float(h[i]) / t if t else 0.0) for i, k in enumerate(ks)}


def label_hit_rate(model, labels, starts_ends_tes, ks, by="mass", exclude=None):
    """Next-category / next-region accuracy: the share of the held-out check-ins (tes_buys_masks under tes_masks) whose LABEL is among
    the top-k labels of model.recommend_labels, for every k in ks (strictly ascending, 1 <= k <= 32).  labels: a PoiLabels; by: "mass"
    (the label's softmax mass) or "max" (its single best POI) - run both to see what the mass buys.  A held-out POI outside [0, n_item)
    or without a label leaves the mean.  All cut-offs come from ONE call at max(ks).  Returns {k: hit rate}."""
    import torch
    ks = [int(k) for k in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] <= 0:
        raise ValueError("ks must be strictly ascending cut-offs >= 1 (got %r)" % (ks,))
    N = model.n_item
    hits = torch.zeros(len(ks), dtype=torch.float64, device=model.device)
    total = torch.zeros((), dtype=torch.float64, device=model.device)
    for se in coalesce_ranges(starts_ends_tes):
        top = model.recommend_labels(se, ks[-1], labels, by=by, exclude=exclude)[0]
        ids, lo = model._ids(se)
        tgt = model._rows(model.tes_buys_masks, ids, lo).long()
        ok = (model._rows(model.tes_masks, ids, lo) != 0) & (tgt >= 0) & (tgt < N)
        want = labels.labels[tgt.clamp(0, N - 1)]                    # (n, len_t) labels of the held-out POIs
        ok &= (want >= 0) & (want < labels.n_label)
        total += ok.sum()
        eq = top[:, None, :] == want[:, :, None]
        found = eq.any(2) & ok
        pos = eq.int().argmax(2)
        for i, k in enumerate(ks):
            hits[i] += (found & (pos < k)).sum()
    h, t = hits.cpu().numpy(), float(total.item())
    return {k: (float(h[i]) / t if t else 0.0) for i, k in enumerate(ks)}


def two_stage_metrics(retriever, ranker, starts_ends_tes, cands=(100, 1000), ks=(5, 10, 20), exclude="train"):
    """What a two-stage recommender loses against its ranker run over ALL POIs: `retriever` hands its top-c candidates
    (compute_sub_candidates) to `ranker`, which scores exactly those and orders them (rerank).  For every candidate cut c in cands
    (strictly ascending, <= min(4096, n_item)) and cut-off k in ks (strictly ascending, k <= cands[0]) the result holds
      out[c]["retriever"] / ["ranker"]   dict(mrr, recall={k: ..}) of each model alone, from the exact ranks of the held-out POIs among
                                         all POIs (compute_sub_target_rank) - the same numbers under every c
      out[c]["two_stage"]                the same for retrieve-then-rerank: a held-out POI outside the c candidates is a miss
                                         (reciprocal rank 0), one inside has the rank of its place in the re-ranked list
      out[c]["agreement"]                {k: share of rows whose two-stage top-k IS the ranker's own top-k over all POIs}
    ONE compute_sub_candidates call of the retriever at max(cands): the smaller cuts are prefixes of its sorted lists.  The held-out
    POIs are the ranker's test rows; one that is excluded (or masked) is not ranked and leaves every mean.  Both models must agree on
    n_item and n_user (ValueError).  The reductions are torch ops on the models' device; scalars reach the host."""
    import torch
    cands, ks = [int(c) for c in cands], [int(k) for k in ks]
    for name, v in (("cands", cands), ("ks", ks)):
        if not v or any(b <= a for a, b in zip(v, v[1:])) or v[0] <= 0:
            raise ValueError("%s must be strictly ascending and >= 1 (got %r)" % (name, v))
    if ks[-1] > cands[0]:
        raise ValueError("every cut-off of ks must be <= the smallest candidate cut (%d > %d)" % (ks[-1], cands[0]))
    if retriever.n_item != ranker.n_item or retriever.n_user != ranker.n_user:
        raise ValueError("retriever and ranker must share the POI table and the user ids (n_item %d vs %d, n_user %d vs %d)"
                         % (retriever.n_item, ranker.n_item, retriever.n_user, ranker.n_user))
    dev = ranker.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    acc = {c: dict(rr=z(), hit=z(len(ks)), same=z(len(ks))) for c in cands}
    alone = {who: dict(rr=z(), hit=z(len(ks))) for who in ("retriever", "ranker")}
    total, rows = z(), 0
    for se in coalesce_ranges(starts_ends_tes):
        ids, lo = ranker._ids(se)
        n = ids.numel()
        if not n:
            continue
        rows += n
        tgt, tm = ranker._rows(ranker.tes_buys_masks, ids, lo), ranker._rows(ranker.tes_masks, ids, lo)
        r_rank = ranker.compute_sub_target_rank(se, exclude=exclude, targets=(tgt, tm)).long()
        ok = r_rank >= 0
        total += ok.sum()
        for who, rk in (("retriever", retriever.compute_sub_target_rank(se, exclude=exclude, targets=(tgt, tm)).long()), ("ranker", r_rank)):
            alone[who]["rr"] += torch.where(ok & (rk >= 0), 1.0 / (rk.clamp(min=0).double() + 1.0), z()).sum()
            for i, k in enumerate(ks):
                alone[who]["hit"][i] += (ok & (rk >= 0) & (rk < k)).sum()
        pool = retriever.compute_sub_candidates(se, cands[-1], exclude=exclude)
        own = ranker.compute_sub_candidates(se, ks[-1], exclude=exclude)
        for c in cands:
            two = ranker.rerank(se, pool[:, :c].contiguous(), c)
            for o in range(0, n, 2048):                              # (rows, targets, c) comparisons, 2048 rows at a time
                eq = two[o:o + 2048, None, :] == tgt[o:o + 2048, :, None].int()
                found = eq.any(2) & ok[o:o + 2048]
                pos = eq.int().argmax(2)
                acc[c]["rr"] += torch.where(found, 1.0 / (pos.double() + 1.0), z()).sum()
                for i, k in enumerate(ks):
                    acc[c]["hit"][i] += (found & (pos < k)).sum()
            for i, k in enumerate(ks):
                acc[c]["same"][i] += (two[:, :k] == own[:, :k]).all(1).sum()
    t = float(total.item())
    share = lambda v, d: float(v) / d if d else 0.0
    single = {who: dict(mrr=share(a["rr"].item(), t), recall={k: share(a["hit"][i].item(), t) for i, k in enumerate(ks)}) for who, a in alone.items()}
    out = {}
    for c in cands:
        a = acc[c]
        out[c] = dict(retriever=single["retriever"], ranker=single["ranker"],
                      two_stage=dict(mrr=share(a["rr"].item(), t), recall={k: share(a["hit"][i].item(), t) for i, k in enumerate(ks)}),
                      agreement={k: share(a["same"][i].item(), rows) for i, k in enumerate(ks)})
    return out


def audience_recall(model, ks, exclude="train"):
    """Recall of the audience direction: over the held-out (user, test POI) pairs (tes_buys_masks under tes_masks), the share of pairs
    whose user lies inside the top-k audience of the POI (model.recommend_audience), for every k in ks (strictly ascending).  ONE call
    over the distinct test POIs at max(ks): the lists are sorted, so the top-k is their first k columns.  exclude as recommend_audience;
    a pair whose user is excluded from its POI (or whose POI lies outside [0, n_item)) is no candidate and leaves the mean.  Returns
    {k: recall}; the reductions are torch ops on the device."""
    import torch
    ks = [int(k) for k in ks]
    if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] <= 0:
        raise ValueError("ks must be strictly ascending cut-offs >= 1 (got %r)" % (ks,))
    N, U, dev = model.n_item, model.n_user, model.device
    tgt = model.tes_buys_masks.long()
    ok = (model.tes_masks != 0) & (tgt >= 0) & (tgt < N)
    u, c = torch.nonzero(ok, as_tuple=True)
    j = tgt[u, c]
    pois = torch.unique(j)                                           # sorted: a pair's query is its POI's position
    qpos = torch.searchsorted(pois, j)
    if not pois.numel():
        return {k: 0.0 for k in ks}
    q32 = pois.int()
    idx = model.recommend_audience(q32, ks[-1], exclude=exclude).long()
    keep = torch.ones_like(u, dtype=torch.bool)
    eo, ex = model._audience_exclusion(exclude, q32, None, U)
    if eo is not None:                                               # a pair on its query's list: sorted keys query * n_user + user
        eo = eo.long()
        rows = torch.repeat_interleave(torch.arange(pois.numel(), device=dev), eo[1:] - eo[:-1])
        keys = rows * U + ex[int(eo[0]):int(eo[-1])].long()
        want = qpos * U + u
        at = torch.searchsorted(keys, want).clamp(max=max(keys.numel() - 1, 0))
        if keys.numel():
            keep &= keys[at] != want
    hits = torch.zeros(len(ks), dtype=torch.float64, device=dev)
    for o in range(0, u.numel(), 4096):                              # (pairs, k) comparisons, 4096 pairs at a time
        eq = idx[qpos[o:o + 4096]] == u[o:o + 4096, None]
        found = eq.any(1) & keep[o:o + 4096]
        pos = eq.int().argmax(1)
        for i, k in enumerate(ks):
            hits[i] += (found & (pos < k)).sum()
    h, t = hits.cpu().numpy(), float(keep.sum().item())
    return {k: (float(h[i]) / t if t else 0.0) for i, k in enumerate(ks)}


def _covisit_share(voff, vus, a, b):
    """The share of the POI pairs (a[i], b[i]) that share at least one visitor.  (voff, vus): data.visitors_csr - per POI its distinct
    visitors, ascending, so poi * n_user + user is one sorted key array; every visitor of a[i] is looked up among the visitors of b[i]."""
    voff, vus = np.asarray(voff, np.int64), np.asarray(vus, np.int64)
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    if not len(a):
        return 0.0
    if not len(vus):
        return 0.0
    stride = int(vus.max()) + 1
    keys = np.repeat(np.arange(len(voff) - 1), np.diff(voff)) * stride + vus
    ln = voff[a + 1] - voff[a]
    pair = np.repeat(np.arange(len(a)), ln)
    pos = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln - voff[a], ln)
    want = b[pair] * stride + vus[pos]
    at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    hit = np.zeros(len(a), bool)
    hit[pair[keys[at] == want]] = True
    return float(hit.mean())


def similar_covisit_rate(model, k, geo_weight=0.0, scale_km=1.0, seed=0):
    """Do the similar-POI lists mean something?  Over every POI as a query: the share of (POI, similar POI) pairs
    (model.similar_pois at k) that share at least one TRAIN visitor (data.visitors_csr), and beside it the same share for k random
    other POIs per query, drawn under a fixed seed.  Returns dict(similar=, random=, pairs= the listed pairs)."""
    from .data import visitors_csr
    n = model.n_item
    voff, vus = visitors_csr(model._off_host, model.p.cpu().numpy(), n)
    pois = np.arange(n)
    idx = model.similar_pois(pois, k, geo_weight=geo_weight, scale_km=scale_km).cpu().numpy().astype(np.int64)
    q = np.repeat(pois, idx.shape[1]).reshape(idx.shape)
    listed = idx >= 0
    rnd = np.random.default_rng(seed).integers(0, max(n - 1, 1), idx.shape)
    rnd = np.minimum(rnd + (rnd >= q), n - 1)                       # (any POI but the query itself)
    return dict(similar=_covisit_share(voff, vus, q[listed], idx[listed]), random=_covisit_share(voff, vus, q[listed], rnd[listed]),
                pairs=int(listed.sum()))


def attribution_by_recency(model, starts_ends, k, explain=None):
    """How far back does a recommendation look?  Every user's own top-k is attributed to their train check-ins (models.Explainer(model).explain
    - or the callable `explain` of the same form - leave-one-out, by="checkin"); check-in t of a history of length L gets the share sum_c |delta[t, c]| / sum_{t', c} |delta[t', c]|
    of the user's attribution.  Returns dict(share= the mean share by position counted from the END (share[0]: the last check-in),
    over the users who have that position, count= those users per position, rows= the users counted: the ones with a history and
    any attribution at all)."""
    if explain is None:
        from .models import Explainer
        explain = Explainer(model).explain
    tot, cnt, rows = np.zeros(0), np.zeros(0, np.int64), 0
    for se in coalesce_ranges(starts_ends):
        out = explain(se, model.compute_sub_topk(se, k))
        delta, off = (np.asarray(t.cpu().numpy()) for t in out[1:3])
        if not len(delta):
            continue
        mass = np.nansum(np.abs(delta), axis=1)
        row = np.repeat(np.arange(len(off) - 1), np.diff(off))
        whole = np.bincount(row, weights=mass, minlength=len(off) - 1)
        live = whole[row] > 0
        from_end = (off[1:][row] - 1 - np.arange(len(mass)))[live]
        n_pos = max(len(tot), int(from_end.max()) + 1 if live.any() else 0)
        tot, cnt = np.pad(tot, (0, n_pos - len(tot))), np.pad(cnt, (0, n_pos - len(cnt)))
        tot += np.bincount(from_end, weights=(mass / np.maximum(whole[row], 1e-300))[live], minlength=n_pos)
        cnt += np.bincount(from_end, minlength=n_pos)
        rows += int((whole > 0).sum())
    return dict(share=tot / np.maximum(cnt, 1), count=cnt, rows=rows)


def foldin_rank_metrics(model, histories, targets, at_nums, exclude="history", **fold_in_kwargs):
    """full_rank_metrics for HELD-OUT users of the factorisation family, of the successive-POI models OboFpmc_lr / OboPrme and of
    OboPoi2vec (strong generalisation): every history is folded in (model.rank_new: fold_in, then the exact rank of its targets among all POIs) and the
    same reductions run on those ranks.  targets: (n, len_t <= 8) POI ids or a pair (ids, mask); exclude: "history" (default), None or
    CSR lists.  OboPrme's gaps= (and dists=) and OboPoi2vec's contexts= travel in fold_in_kwargs.  Returns the keys of full_rank_metrics; ndcg is averaged over
    the n histories."""
    rank, cnt = model.rank_new(histories, targets=targets, exclude=exclude, return_counts=True, **fold_in_kwargs)
    return _metrics_of_ranks(model, [(rank, cnt)], at_nums, rank.shape[1], rank.shape[0])


def _metrics_of_ranks(model, batches, at_nums, lt, n_user):
    """The reductions of full_rank_metrics over (rank (n, lt), count (n)) device batches."""
    import torch
    at_nums = list(at_nums)
    if any(b <= a for a, b in zip(at_nums, at_nums[1:])) or (at_nums and (at_nums[0] <= 0 or at_nums[-1] > model.n_item)):
        raise ValueError("at_nums must be strictly ascending cut-offs in [1, n_item] (got %r)" % (at_nums,))
    dev = model.device
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    acc = f64(4)                                  # valid positions, sum 1 / (rank + 1), sum rank, sum auc term
    hits, ndcg = f64(len(at_nums)), f64(len(at_nums))
    disc_cum = torch.cat([f64(1), torch.cumsum(1.0 / torch.log2(torch.arange(lt, device=dev, dtype=torch.float64) + 2.0), 0)])      # ideal DCG of m hits
    kept = []
    for rank, cnt in batches:
        ok = rank >= 0
        r = rank.double()
        c = cnt.double()[:, None].expand_as(r)
        acc += torch.stack([ok.sum().double(), torch.where(ok, 1.0 / (r + 1.0), f64(1)).sum(), torch.where(ok, r, f64(1)).sum(),
                            torch.where(ok, torch.where(c > 1, 1.0 - r / (c - 1.0).clamp(min=1.0), f64(1) + 1.0), f64(1)).sum()])
        n_test = ok.sum(1)
        for i, k in enumerate(at_nums):
            hit = ok & (rank < k)
            dcg = torch.where(hit, 1.0 / torch.log2(r.clamp(min=0) + 2.0), f64(1)).sum(1)
            ideal = disc_cum[n_test.clamp(max=min(k, lt))]
            hits[i] += hit.sum(); ndcg[i] += torch.where(hit.any(1), dcg / ideal.clamp(min=1e-300), f64(1)).sum()
        kept.append(rank[ok])
    allr = torch.cat(kept) if kept else torch.zeros(0, dtype=torch.int32, device=dev)
    med = float(torch.sort(allr)[0][(allr.numel() - 1) // 2].item()) if allr.numel() else 0.0
    a, h, g = acc.cpu().numpy(), hits.cpu().numpy(), ndcg.cpu().numpy()
    n = float(a[0])
    out = dict(n=n, mrr=float(a[1] / n) if n else 0.0, mean_rank=float(a[2] / n) if n else 0.0, median_rank=med,
               auc_full=float(a[3] / n) if n else 0.0, at={})
    for i, k in enumerate(at_nums):
        out["at"][k] = dict(hits=float(h[i]), recall=float(h[i] / n) if n else 0.0, ndcg=float(g[i]) / n_user)
    return out


def fun_predict_auc_recall_map_ndcg(p, model, best, epoch, starts_ends_auc, starts_ends_tes, tes_buys_masks, tes_masks, on_device=True):
    """Same signature and side effects on `best` as public/Valuate.py:103-191; returns the metrics too.
    With on_device (default) the ranks never leave the GPU; on_device=False downloads them and uses the
    vectorised numpy restatement (rank_metrics) - both are tested against the reference's helpers."""
    at_nums = p["at_nums"]
    upqs = np.concatenate([model.compute_sub_auc_preference(se) for se in starts_ends_auc])
    auc = float(upqs.sum()) / float(np.sum(tes_masks))             # Valuate.py:113-118
    if auc > best.best_auc:
        best.best_auc, best.best_epoch_auc = auc, epoch
    kmax = at_nums[-1]
    if on_device:
        all_ranks = None
        m = device_rank_metrics(model, starts_ends_tes, at_nums)
    else:
        all_ranks = np.concatenate([model.compute_sub_topk(se, kmax).cpu().numpy() for se in starts_ends_tes])
        m = rank_metrics(all_ranks, tes_buys_masks, tes_masks, at_nums)
    for i, k in enumerate(at_nums):
        for name, key in (("recall", "recall"), ("precis", "precision"), ("f1scor", "f1"), ("map", "map"), ("ndcg", "ndcg")):
            cur = getattr(best, "best_" + name)
            if m[k][key] > cur[i]:
                cur[i] = m[k][key]
                getattr(best, "best_epoch_" + name)[i] = epoch
    return dict(auc=auc, at=m, ranks=all_ranks)


def intra_list_distance_km(idx, coords):
    """Mean pairwise great-circle distance (km) within each recommendation list: idx (n, k) POI ids with -1 for an empty place (ignored),
    coords (n_item, 2) lat, lon.  Returns (n) float64, NaN for a list of fewer than two POIs.  The distance is the sin^2 Haversine form
    of the re-ranking (include/poi_hip.h, poi_diverse_rerank).  With catalogue_coverage, the number that shows what diversification did."""
    idx = np.asarray(idx.cpu().numpy() if hasattr(idx, "cpu") else idx, np.int64)
    xy = np.asarray(coords.cpu().numpy() if hasattr(coords, "cpu") else coords, np.float64)
    idx = idx.reshape(len(idx), -1)
    ok = idx >= 0
    g = np.where(ok, idx, 0)
    lat, lon = xy[g, 0], xy[g, 1]
    cp = np.cos(lat * (np.pi / 180.0))
    sa = np.sin((lat[:, :, None] - lat[:, None, :]) * (np.pi / 360.0))
    sb = np.sin((lon[:, :, None] - lon[:, None, :]) * (np.pi / 360.0))
    d = 12742.0 * np.arcsin(np.minimum(1.0, np.sqrt(sa * sa + cp[:, :, None] * cp[:, None, :] * (sb * sb))))
    pair = ok[:, :, None] & ok[:, None, :] & np.triu(np.ones((idx.shape[1], idx.shape[1]), bool), 1)[None]
    cnt = pair.sum(axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, (d * pair).sum(axis=(1, 2)) / cnt, np.nan)


def catalogue_coverage(idx, n_item):
    """Fraction of the catalogue's n_item POIs that appear on at least one of the lists idx (n, k); -1 places are ignored."""
    idx = np.asarray(idx.cpu().numpy() if hasattr(idx, "cpu") else idx, np.int64).reshape(-1)
    idx = idx[(idx >= 0) & (idx < n_item)]
    return float(np.unique(idx).size) / float(n_item)


def label_spread(idx, labels):
    """What a cap did to recommendation lists: idx (n, k) POI ids with -1 for an empty place (ignored), labels (n_item) ints (< 0:
    unlabelled, every such POI a group of its own) -> (distinct (n) int64: the number of distinct labels on each list; share (n)
    float64: the largest fraction of a list that one label holds, NaN for an empty list).  A per = 1 list has share 1 / its length.
    With intra_list_distance_km and catalogue_coverage, the figures of the re-ranked and the capped lists."""
    idx = np.asarray(idx.cpu().numpy() if hasattr(idx, "cpu") else idx, np.int64)
    lab = np.asarray(labels.cpu().numpy() if hasattr(labels, "cpu") else labels, np.int64)
    idx = idx.reshape(len(idx), -1)
    distinct, share = np.zeros(len(idx), np.int64), np.full(len(idx), np.nan)
    for r, row in enumerate(idx):
        ids = row[row >= 0]
        if not ids.size:
            continue
        l = lab[ids]
        groups = np.where(l >= 0, l, -1 - ids)                  # an unlabelled POI: a group of its own
        _, cnt = np.unique(groups, return_counts=True)
        distinct[r], share[r] = cnt.size, cnt.max() / ids.size
    return distinct, share
