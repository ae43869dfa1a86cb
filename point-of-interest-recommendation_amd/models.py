"""Host-side mirror of the reference's model-object protocol on top of libpoi_hip.so.

Class / method names, argument meaning and return shapes follow the Theano classes the drivers call:
    OboSpatialGru  public/GRU_Spatial.py:42-292      OboGru  public/GRU.py:301-389 (+ GruBasic :32-205)
    Gru / Lstm / Rnn  public/GRU.py:395-498 / :502-657 / :661-809 (the mini-batch classes)
    OboBpr         public/BPR.py:191-241 (+ MfBasic :28-134)      OboVBpr  public/BPR.py:245-335
so that prog_bpr_gru_spatial.py's epoch loop and public/Valuate.py's evaluator run against them
unchanged in shape.  State lives in torch ROCm tensors (device-memory containers only); every piece of
arithmetic is a HIP kernel reached through ctypes.  There is no CPU path: without the library or a GPU
the constructors raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .data import CsrTables, bin_thresholds, cos_lat, padded_to_csr


import os

_CHECK_DEVICE_IDS = os.environ.get("POI_CHECK_IDS", "0") == "1"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _at(t, o, w):
    """Row o of a row-major tensor of w columns as a pointer (None stays None): where a chunk of rows writes its part of an output."""
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * o * w) if t is not None else None


class ScoreSource:
    """What a per-row serving call ranks - n rows, each with a score for every POI - and nothing else.  A FUSED source scores by
    users . items (+ the spatial distance term) inside the serving kernels; any other one hands out explicit score rows, a bounded
    number at a time.  Three producers: _Base._source (trained users), Session._source (live slots), CellSession._source (CA-RNN's
    own rule).  The per-row families (_Base._serve_*) are written once over a source.

    fused sources:  users (n, kdim) float32 contiguous, items, kdim, tile_term(clamp, pad) -> (wd, sts rows, last POI rows) | None as
                    _tile_operands takes it, near_term() -> (wd, sts rows, thr, n_dist, dd_m) | None as _near_launch takes it - each
                    built when it is asked for.
    other sources:  score_rows(positions=False) -> rows(o, c), the (c, n_item) scores of rows o .. o + c - 1 (positions: every
                    (row, position) row of a model that scores them, row-major).
    every source:   anchor() -> the default anchor rows (the last train POI / the slot's last_poi, -1: none); exclusion(exclude);
                    finish(out, ...); need_fused(family)."""

    def __init__(self, model, n, kinds, anchor, refusals, ids=None, lo=None, users=None, items=None, tile_term=None, near_term=None,
                 score_rows=None, has=None):
        self.m, self.n, self.kinds, self.anchor, self.refusals, self.ids, self.lo = model, n, kinds, anchor, refusals, ids, lo
        self.fused = users is not None
        self.users, self.items, self.kdim = users, items, (model.kdim if self.fused else None)
        self._tile_term, self._near_term, self.score_rows, self.has = tile_term, near_term, score_rows, has

    def tile_term(self, clamp=False, pad=False):
        """clamp: the last POI rows clamped to 0 (the kernel relies on the zero sts row: target ranks, the unrestricted top-K);
        pad: sts rows padded to whole 32-row tiles (poi_score_topk_geo alone).  Both mean something to a session only."""
        return self._tile_term(clamp, pad)

    def near_term(self):
        return self._near_term()

    def need_fused(self, family):
        """A call that needs users . items on a source that ranks by a rule of its own: PoiError, the producer's text."""
        if not self.fused:
            raise _lib.PoiError(self.refusals()[family])

    def exclusion(self, exclude, anchor=None):
        """exclude -> (off (n + 1), ids) int32 device tensors or (None, None): None, one of the source's names - "train" (the users'
        distinct train POIs: a contiguous user range windows the cached CSR), "last" (`anchor`, default the source's own) - or CSR
        lists (off, ids).  Any other name raises ValueError with the names this source accepts."""
        if anchor is None and isinstance(exclude, str) and exclude == "last" and "last" in self.kinds:
            anchor = self.anchor()
        return self.m._near_exclusion(exclude, self.n, anchor, self.ids, self.lo, self.kinds)

    def finish(self, out, return_scores, return_counts, ranked=False):
        """ids-or-ranks[, scores][, ...][, counts] as the caller gets them: the identity, except for a CA-RNN session - a slot without
        a check-in (`has` false; its row was scored at POI 0 and masked to -inf) counts 0 candidates, and `ranked` (recommend,
        rank_of: the kernel ranks the masked row all the same) also gives it -1 and a NaN score."""
        has = self.has
        if has is None:
            return out
        out = list(out) if isinstance(out, tuple) else [out]
        if ranked:
            out[0] = torch.where(has[:, None], out[0], torch.full_like(out[0], -1))
            if return_scores:
                out[1] = torch.where(has[:, None], out[1], torch.full_like(out[1], float("nan")))
        if return_counts:
            out[-1] = torch.where(has, out[-1], torch.zeros_like(out[-1]))
        return tuple(out) if len(out) > 1 else out[0]


class Shared:
    """Stand-in for a Theano shared variable: .get_value() / .set_value() on a device tensor."""

    def __init__(self, tensor, scalar=False, pad=None, unpad=None):
        self.t = tensor
        self.scalar = scalar
        self.pad, self.unpad = pad, unpad      # logical <-> stored layout (models whose dim is padded to a tile-engine dim)

    def get_value(self, borrow=False):
        a = self.t.detach().cpu().numpy()
        if self.unpad is not None:
            a = np.ascontiguousarray(self.unpad(a))
        return a.reshape(()).copy() if self.scalar else a

    def set_value(self, value, borrow=False):
        v = np.asarray(value, dtype=np.float64)
        if self.pad is not None:
            v = self.pad(v)
        v = torch.as_tensor(v, dtype=self.t.dtype).reshape(self.t.shape)
        self.t.copy_(v.to(self.t.device))


class _L2:
    """model.l2 - an object with .eval() (public/GRU_Spatial.py:83-88)."""

    def __init__(self, model, names):
        self.model, self.names = model, names

    def eval(self):
        m = self.model
        acc = torch.zeros(1, dtype=torch.float64, device=m.device)
        for n in self.names:
            t = getattr(m, n).t
            m.ctx.check(m.lib.poi_sumsq(m.ctx.handle, _ptr(t), t.numel(), _ptr(acc), m._stream()))
        return 0.5 * m.alpha_lambda[1] * float(acc.item())


class PoiFilter:
    """Pass bitmaps of P predicates over a model's POIs (include/poi_hip.h, poi_filter_build): `bits` (P, W = ceil(n_item / 32)) int32
    on the device - POI j is bit j & 31 of word j >> 5 of its predicate's row - and `counts` (P) on the host, the POIs each predicate
    passes.  Built by model.poi_filter(predicates) from the model's attributes, or from boolean masks of the caller's own
    (from_masks: a predicate the attribute words cannot express, such as opening hours evaluated at query time)."""

    def __init__(self, model, bits, counts):
        self.n_item, self.bits, self.counts = model.n_item, bits, np.asarray(counts, np.int64)
        self.n_pred, self.ldw = int(bits.shape[0]), int(bits.shape[1])

    @classmethod
    def from_masks(cls, model, masks):
        """masks: boolean (P, n_item) (or (n_item)), numpy or torch - packed by data.pack_pass_bits."""
        from .data import pack_pass_bits
        m = masks if isinstance(masks, torch.Tensor) else np.asarray(masks)
        m = m.reshape(1, -1) if m.ndim == 1 else m
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] != model.n_item:
            raise ValueError("masks must be (P >= 1, n_item = %d) (got %s)" % (model.n_item, tuple(m.shape)))
        if isinstance(m, torch.Tensor):
            return cls(model, pack_pass_bits(m).to(model.device).contiguous(), (m != 0).sum(dim=1).cpu().numpy())
        bits = torch.as_tensor(pack_pass_bits(m).view(np.int32)).to(model.device).contiguous()
        return cls(model, bits, (m != 0).sum(axis=1))


class PoiLabels:
    """A labelling of a model's POIs for the capped top-K (include/poi_hip.h, poi_labels_build): `labels` (n_item) int32 on the device
    (>= 0: the POI's group; < 0: unlabelled, a group of its own that is never capped), `fill` (P, 33) int32 on the device - the longest
    list predicate q of `filt` (one row without a filter) can give under a cap of m, the gate of compute_sub_topk_capped - and
    `counts` (n_label) on the host, the POIs of every label.  Built by model.poi_labels(labels) or from_categories(model)."""

    def __init__(self, model, labels, n_label, fill, counts, filt=None):
        self.n_item, self.labels, self.n_label, self.fill, self.filt = model.n_item, labels, int(n_label), fill, filt
        self.counts = np.asarray(counts, np.int64)

    @classmethod
    def from_categories(cls, model, filt=None):
        """The categories of model.set_attributes as the labels (n_label = n_cat)."""
        cat, _, n_cat = model.__dict__.get("_attr", (None, None, 1))
        if cat is None:
            raise _lib.PoiError("the model holds no categories: call set_attributes(categories=...) first")
        return model.poi_labels(cat, n_cat, filt)


class _Base:
    def _setup(self, device, alpha_lambda):
        if not torch.cuda.is_available():
            raise _lib.PoiError("no ROCm device visible: the next-POI hot path has no CPU implementation")
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.ctx = _lib.context(idx)
        self.lib = self.ctx.lib
        self.alpha_lambda = [float(alpha_lambda[0]), float(alpha_lambda[1])]

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):          # (a device tensor is taken as it is: 10 M-row tables are generated on the device)
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(self.device).contiguous()

    def _ids(self, idxs):
        """(int32 device tensor of user ids, lo) - lo is the first id when the ids are a contiguous
        ascending range (then the tensor is a zero-copy view of a resident arange), else None.
        Host ids (scalars, lists, numpy) are range-checked and raise IndexError like the reference's Theano
        gather - the kernels would read off[u] out of bounds.  A DEVICE tensor is trusted (checking it
        costs a host sync per launch); set POI_CHECK_IDS=1 to check those too."""
        if isinstance(idxs, torch.Tensor):
            t = idxs.to(device=self.device, dtype=torch.int32).contiguous()
            if _CHECK_DEVICE_IDS and t.numel():
                lo_, hi_ = int(t.min().item()), int(t.max().item())
                if lo_ < 0 or hi_ >= self.n_user:
                    raise IndexError("user ids must lie in [0, %d) (found %d..%d)" % (self.n_user, lo_, hi_))
            return t, None
        a = np.atleast_1d(np.asarray(idxs)).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_user):
            raise IndexError("user ids must lie in [0, %d) (found %d..%d)" % (self.n_user, int(a.min()), int(a.max())))
        if len(a) and np.all(np.diff(a) == 1):
            lo = int(a[0])
            return self._arange[lo:lo + len(a)], lo
        return torch.as_tensor(a.astype(np.int32)).to(self.device), None

    def _rows(self, table, ids, lo):
        n = ids.numel()
        return table[lo:lo + n] if lo is not None else table.index_select(0, ids.long()).contiguous()

    def _by_length(self, idxs):
        """(ids sorted by descending sequence length, out_row) for the recurrent kernels: a 16-sequence tile runs for
        its longest member, so homogeneous tiles halve the forward pass of a full evaluation.  out_row[k] = position of
        the k-th sorted id in the caller's order: poi_gru_predict writes its result there, so nothing is permuted
        afterwards.  The order is computed on the host from the host-side lengths (once per distinct id list: cached for
        the common "all users" / contiguous-range calls).  Device tensors and small launches are taken as they come."""
        if isinstance(idxs, torch.Tensor):
            return self._ids(idxs)[0], None
        a = np.atleast_1d(np.asarray(idxs)).astype(np.int64)
        ids, lo = self._ids(a)
        if len(a) < 64:
            return ids, None
        key = (int(a[0]), len(a)) if lo is not None else None
        cache = self.__dict__.setdefault("_order_cache", {})
        if key is not None and key in cache:
            return cache[key]
        order = np.argsort(-np.asarray(self._lens)[a], kind="stable").astype(np.int32)
        out = (torch.as_tensor(a[order].astype(np.int32)).to(self.device), torch.as_tensor(order).to(self.device))
        if key is not None and len(cache) < 64:
            cache[key] = out
        return out

    # ---- tables -------------------------------------------------------------------------------
    @staticmethod
    def _check_ids(name, ids, hi):
        """The reference gathers with Theano advanced indexing, which raises IndexError on an id outside the
        table; the kernels would read out of bounds - so ids are checked where they enter."""
        a = np.asarray(ids)
        if a.size and (a.min() < 0 or a.max() > hi):
            raise IndexError("%s: ids must lie in [0, %d] (found %d..%d)" % (name, hi, int(a.min()), int(a.max())))

    # ---- fold-in glue shared by MfBasic and the successive-POI models -------------------------------------------------------------
    def _foldin_csr(self, histories):
        """histories -> (off (n + 1), p) int32 device tensors, n, total.  A tuple (off, p_flat) is a CSR, anything else a list of id
        sequences.  Host data is checked here (IndexError / ValueError before any launch); of a device CSR only the offsets' range is
        checked (one sync: they address memory), its ids and the order of its offsets are left to the kernel."""
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        if isinstance(histories, tuple) and len(histories) == 2:
            off, p = histories
            if isinstance(off, torch.Tensor) and isinstance(p, torch.Tensor) and p.is_cuda:
                off = off.to(self.device, torch.int32).contiguous().reshape(-1)
                p = p.to(self.device, torch.int32).contiguous().reshape(-1)
                if off.numel() < 1:
                    raise ValueError("histories=(off, p_flat): off must hold n + 1 offsets")
                lo, hi, first, last = (int(v) for v in torch.stack([off.min(), off.max(), off[0], off[-1]]).cpu())
                if lo < 0 or hi > p.numel():
                    raise IndexError("histories=(off, p_flat): offsets must lie in [0, %d] (found %d..%d)" % (p.numel(), lo, hi))
                if first != 0 or last != p.numel():
                    raise ValueError("histories=(off, p_flat): off must run from 0 to len(p_flat)")
                return off, (p if p.numel() else torch.zeros(1, dtype=torch.int32, device=self.device)), off.numel() - 1, p.numel()
            off = np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off).astype(np.int64).reshape(-1)
            p = np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p).astype(np.int64).reshape(-1)
            if off.size < 1 or off[0] != 0 or off[-1] != p.size or np.any(np.diff(off) < 0):
                raise ValueError("histories=(off, p_flat): off must ascend from 0 to len(p_flat)")
        else:
            seqs = [np.asarray(h, np.int64).reshape(-1) for h in histories]
            off = np.zeros(len(seqs) + 1, np.int64)
            off[1:] = np.cumsum([len(s) for s in seqs])
            p = np.concatenate(seqs) if seqs else np.zeros(0, np.int64)
        if p.size >= (1 << 31):
            raise ValueError("fold_in: at most 2^31 - 1 check-ins per call")
        self._check_ids("fold_in histories", p, self.n_item)
        return i32(off), i32(p if p.size else [0]), len(off) - 1, int(p.size)

    def _foldin_exclusion(self, exclude, off, p, n, total):
        """exclude -> (ex_off, ex): "history" = every history's distinct POIs, ascending (the padding id n_item is no candidate and
        is dropped); None or a CSR pair as compute_sub_topk_near."""
        if not isinstance(exclude, str):
            return self._near_exclusion(exclude, n, None)
        if exclude != "history":
            raise ValueError("exclude must be None, 'history' or a pair (off, ids) (got %r)" % (exclude,))
        o = off.long()
        row = torch.repeat_interleave(torch.arange(n, device=self.device), o[1:] - o[:-1])
        ids = p[:total].long()
        keys = torch.unique((row * (self.n_item + 1) + ids)[ids < self.n_item])             # sorted: by row, then by id
        eo = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        eo[1:] = torch.cumsum(torch.bincount(keys // (self.n_item + 1), minlength=n), 0)
        ex = (keys % (self.n_item + 1)).int()
        return eo.int(), (ex if ex.numel() else torch.zeros(1, dtype=torch.int32, device=self.device))

    def _foldin_init(self, init, n, dim, mean_of):
        """init -> the (n, dim) start rows on the device, or None for zeros: "zeros", "mean" (the mean row of `mean_of`) or an array."""
        if isinstance(init, str):
            if init not in ("zeros", "mean"):
                raise ValueError("init must be 'zeros', 'mean' or an (n, kdim) array (got %r)" % (init,))
            return None if init == "zeros" else mean_of.mean(0, keepdim=True).expand(n, dim).contiguous()
        w0 = self._dev(init).reshape(-1, dim)
        if w0.shape[0] != n:
            raise ValueError("init must hold one row per history (%d vs %d)" % (w0.shape[0], n))
        return w0

    def _foldin_given_negatives(self, negatives, total, epochs, lo=0):
        """Explicit negatives -> (q int32 device, q_epoch_stride): `total` ids (one draw for every epoch) or epochs x total, epoch-major.
        Host arrays are range-checked ([lo, n_item]) before any launch; device tensors are left to the kernel."""
        if isinstance(negatives, torch.Tensor) and negatives.is_cuda:
            q = negatives.to(self.device, torch.int32).contiguous().reshape(-1)
        else:
            qh = np.asarray(negatives.cpu() if isinstance(negatives, torch.Tensor) else negatives).astype(np.int64).reshape(-1)
            self._check_ids("fold_in negatives", qh if lo == 0 else qh[qh != -1], self.n_item)
            q = torch.as_tensor(qh.astype(np.int32)).to(self.device)
        if q.numel() == total:
            stride = 0
        elif q.numel() == epochs * total:
            stride = total
        else:
            raise ValueError("negatives must hold total = %d or epochs x total = %d ids (got %d)" % (total, epochs * total, q.numel()))
        if not q.numel():
            q = self._some_ids()
        return q, stride

    def _load_tables(self, train, test):
        self._csr = train if isinstance(train, CsrTables) else None
        if self._csr is not None:
            c = self._csr
            off = np.ascontiguousarray(c.off, np.int32)
            self._check_ids("train POIs", c.p, self.n_item); self._check_ids("train negatives", c.q, self.n_item)
            self._check_ids("test POIs", c.tes_p, self.n_item); self._check_ids("test negatives", c.tes_q, self.n_item)
            self._lens = np.diff(off.astype(np.int64))
            self.len_max, self.max_len = int(c.len_max), int(self._lens.max())
            self._off_host = off
            i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
            self.off, self.p, self.q = i32(off), i32(c.p), i32(c.q)
            self.tes_buys_masks, self.tes_masks, self.tes_buys_neg_masks = i32(c.tes_p), i32(c.tes_mask), i32(c.tes_q)
            self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)
            return
        tra_buys_masks, tra_masks, tra_buys_neg_masks = train
        tes_buys_masks, tes_masks, tes_buys_neg_masks = test
        for nm, t in (("train POIs", tra_buys_masks), ("train negatives", tra_buys_neg_masks), ("test POIs", tes_buys_masks),
                      ("test negatives", tes_buys_neg_masks)):
            self._check_ids(nm, t, self.n_item)
        tra_masks = np.asarray(tra_masks)
        self._lens = tra_masks.sum(axis=1).astype(np.int64)
        self.len_max = int(tra_masks.shape[1])                 # padded length LM of the reference tables
        self.max_len = int(self._lens.max())
        off, p = padded_to_csr(tra_buys_masks, self._lens)
        _, q = padded_to_csr(tra_buys_neg_masks, self._lens)
        self._off_host = off
        self.off, self.p, self.q = (torch.as_tensor(v).to(self.device) for v in (off, p, q))
        self.tes_buys_masks = self._dev(tes_buys_masks, torch.int32)
        self.tes_masks = self._dev(tes_masks, torch.int32)
        self.tes_buys_neg_masks = self._dev(tes_buys_neg_masks, torch.int32)
        self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)

    def update_neg_masks(self, tra_buys_neg_masks, tes_buys_neg_masks):
        """public/GRU.py:79-82 / public/BPR.py:61-64 - new negatives every epoch."""
        self._check_ids("train negatives", tra_buys_neg_masks, self.n_item); self._check_ids("test negatives", tes_buys_neg_masks, self.n_item)
        _, q = padded_to_csr(tra_buys_neg_masks, self._lens)
        self.q = torch.as_tensor(q).to(self.device)
        self.tes_buys_neg_masks = self._dev(tes_buys_neg_masks, torch.int32)

    def set_negatives_csr(self, q_flat, tes_q=None, dq_flat=None):
        """CSR form of update_neg_masks / s_update_neg_masks (no padded tables built)."""
        self.q = torch.as_tensor(np.ascontiguousarray(q_flat, dtype=np.int32)).to(self.device)
        if tes_q is not None:
            self.tes_buys_neg_masks = self._dev(np.asarray(tes_q).reshape(self.n_user, -1), torch.int32)
        if dq_flat is not None:
            self.dq = torch.as_tensor(np.ascontiguousarray(dq_flat, dtype=np.int32)).to(self.device)

    def resample_negatives_device(self, seed):
        """Per-epoch negative refresh entirely on the device (prog_bpr_gru_spatial.py:221-228): new train /
        test negatives (Load_Data_by_length.py:127-162) and, for the spatial model, their distance bins
        (:165-180).  No host work, no upload; reproducible for a given seed."""
        q = torch.empty_like(self.p)
        tq = torch.empty_like(self.tes_buys_masks)
        self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(self.off), _ptr(self.p), self.n_user, self.n_item,
                                                     _ptr(self.tes_buys_masks), _ptr(self.tes_masks), self.tes_masks.shape[1],
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(q), _ptr(tq), self._stream()))
        self.q, self.tes_buys_neg_masks = q, tq
        if getattr(self, "spatial", False):
            if self.coords is None:
                raise _lib.PoiError("resample_negatives_device on the spatial model needs coords= at construction")
            dq = torch.empty_like(self.p)
            self.ctx.check(self.lib.poi_neg_dist_bins(self.ctx.handle, _ptr(self.off), _ptr(self.p), _ptr(self.q), self.n_user,
                                                      _ptr(self.coords), _ptr(self._cphi), _ptr(self._binthr), self.n_dist,
                                                      self.dd * 1000.0, _ptr(dq), self._stream()))
            self.dq = dq

    # ---- snapshots ----------------------------------------------------------------------------
    def update_trained_items(self):
        """public/GRU.py:84-87: eval sees a snapshot of lt, not the live table."""
        self.trained_items.t.copy_(self.lt.t)

    def compute_sub_auc_preference(self, start_end):
        """public/GRU.py:98-110 -> bool ndarray (n, len_tes)."""
        ids, lo = self._ids(start_end)
        n = ids.numel()
        ln = self.tes_masks.shape[1]
        users = self._rows(self.trained_users.t, ids, lo)
        tp, tq, tm = (self._rows(t, ids, lo) for t in (self.tes_buys_masks, self.tes_buys_neg_masks, self.tes_masks))
        out = torch.empty((n, ln), dtype=torch.uint8, device=self.device)
        self.ctx.check(self.lib.poi_auc_preference(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), n, self.kdim,
                                                   _ptr(tp), _ptr(tq), _ptr(tm), ln, _ptr(out), self._stream()))
        return out.cpu().numpy().astype(bool)

    def _users_rows(self, start_end):
        ids, lo = self._ids(start_end)
        return ids, self._rows(self.trained_users.t, ids, lo), lo

    def _items(self):
        """The POI rows the fused serving kernels take the product users . items with."""
        return self.trained_items.t

    def _prob_rows(self, ids, lo):
        return None, None

    def compute_sub_all_scores(self, start_end):
        """public/GRU.py:93-96 (spatial: public/GRU_Spatial.py:117-125) -> ndarray (n, n_item)."""
        return self.compute_sub_all_scores_device(start_end).cpu().numpy()

    def compute_sub_all_scores_device(self, start_end):
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        wd, prob = self._prob_rows(ids, lo)
        out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_score_all(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), n, self.n_item, self.kdim,
                                              _ptr(wd), _ptr(prob), _ptr(out), self._stream()))
        return out

    def compute_sub_topk(self, start_end, k, return_scores=False):
        """Fused a8+a9: (n, k) int32 indices sorted by descending score (public/Valuate.py:132-146)
        without materialising the (n, n_item) score matrix."""
        if k > 32:
            return self._topk_from_scores(start_end, k, return_scores)
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        wd, prob = self._prob_rows(ids, lo)
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
        seed = self._seed_begin(lo, n, k)
        self.ctx.check(self.lib.poi_score_topk(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), n, self.n_item, self.kdim,
                                               _ptr(wd), _ptr(prob), int(k), _ptr(idx), _ptr(sc), self._stream()))
        self._seed_end(seed, idx)
        return (idx, sc) if return_scores else idx

    # Seeded top-K (include/poi_hip.h, poi_ctx_set_topk_seed): the previous evaluation's top-K ids of a contiguous user range seed the
    # thresholds of the next one - exact whatever they hold, several times fewer candidate insertions.  `topk_seeding = False` disables.
    topk_seeding = True

    def _seed_begin(self, lo, n, k):
        if not self.topk_seeding or lo is None or k > 32:
            return None
        seeds = self.__dict__.setdefault("_topk_seeds", {})
        t = seeds.get(int(k))
        if t is None:
            t = seeds[int(k)] = (torch.full((self.n_user, int(k)), -1, dtype=torch.int32, device=self.device), np.zeros(self.n_user, bool))
        rows = t[0][lo:lo + n]
        if t[1][lo:lo + n].all():                 # seed only with lists a previous evaluation wrote (the first one runs unseeded)
            self.ctx.set_topk_seed(rows, k)
        return rows, t[1], lo, n

    def reset_topk_seeds(self):
        """Forget the lists of earlier evaluations (the next one runs unseeded).  (Measured and not kept, round 4: a static prior - the 20 POIs
        nearest to each user's last check-in - as the seed of the first evaluation.  Under a trained model only 24 % of the final top-20 are
        among them: the seed's K-th best is far below the final one, 8600 survivors per user, every tile overflows - 47 ms against 11 ms unseeded.)"""
        self.__dict__.pop("_topk_seeds", None)

    def _seed_end(self, seed, idx):
        if seed is not None:
            rows, filled, lo, n = seed
            rows.copy_(idx)
            filled[lo:lo + n] = True


    # ---- explicit score rows: the models and sessions that rank by a rule of their own build (rows, n_item) float32 scores, a bounded
    # number of rows at a time, and hand them to poi_topk / poi_rank_scores / poi_topk_select / ... ------------------------------------
    SCORE_ROWS_BYTES = 1 << 30      # of score rows alive at a time (an instance may set its own)

    def _rank_chunk(self, n):
        return max(1, min(n, self.SCORE_ROWS_BYTES // (4 * max(self.n_item, 1))))

    def _row_chunks(self, n, step=None):
        """(o, c): rows o .. o + c - 1 of n, _rank_chunk rows at a time."""
        step = step or self._rank_chunk(max(n, 1))
        for o in range(0, n, step):
            yield o, min(step, n - o)

    @staticmethod
    def _id_list(start_end):
        return start_end if isinstance(start_end, torch.Tensor) else np.atleast_1d(np.asarray(start_end))

    def _own_score_rows(self, a, positions=False):
        """score_rows(o, c) -> the model's own score rows (_rank_score_rows) of the users a[o : o + c]: one row per user - of (user,
        position) rows position 0, the user's next POI - or, with `positions`, all of them, user-major."""
        def score_rows(o, c):
            full, per = self._rank_score_rows(a[o:o + c])
            return full.view(c, per, self.n_item)[:, 0] if per > 1 and not positions else full
        return score_rows

    def _refusals(self):
        """What a call that needs users . items says to a model that ranks by a rule of its own (ScoreSource.need_fused)."""
        own = "%s ranks by a score rule of its own, not users . items: " % type(self).__name__
        return {"near": own + "compute_sub_topk_near does not cover it", "filtered": own + "within_km / anchor are not defined for it"}

    def _source(self, start_end, kinds=("train",), fused=None):
        """The ScoreSource of the trained users `start_end`: fused (trained_users rows . _items(), the distance term of _rank_term /
        _near_term) where the model scores by users . items - _rank_fused, read per call: GeoIE's follows its rule - and the model's
        own score rows otherwise.  kinds: the exclude= names the calling family accepts; fused: the family's own condition."""
        refusals = self._refusals                                # (the texts are built when one is raised)
        if not (self._rank_fused if fused is None else fused):
            a = self._id_list(start_end)
            ids, lo = self._ids(a)
            anchor, rows = (lambda: self._rows(self._last_train_poi(), ids, lo)), (lambda positions=False: self._own_score_rows(a, positions))
            return ScoreSource(self, len(a), kinds, anchor, refusals, ids, lo, score_rows=rows)
        ids, users, lo = self._users_rows(start_end)
        return ScoreSource(self, ids.numel(), kinds, lambda: self._rows(self._last_train_poi(), ids, lo), refusals, ids, lo, users.contiguous(),
                           self._items(), lambda clamp, pad: self._rank_term(ids, lo), lambda: self._near_term(ids, lo))

    def _topk_buffers(self, n, k, return_scores, return_counts):
        """(idx (n, k) int32, scores (n, k) float32 | None, counts (n) int32 | None): the outputs of a top-K or rank call."""
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n, dtype=torch.int32, device=self.device) if return_counts else None
        return idx, sc, cnt

    def _some_ids(self, t=None):
        """An int32 id list as the library takes it: `t` itself, a one-element placeholder for an empty (or no) list."""
        return t if t is not None and t.numel() else torch.zeros(1, dtype=torch.int32, device=self.device)

    def _csr_take(self, ids, beg, ln):
        """The lists ids[beg[r] : beg[r] + ln[r]] (int64 device rows) as a CSR of their own: (off (rows + 1) int32, ids)."""
        off = torch.zeros(ln.numel() + 1, dtype=torch.int64, device=self.device)
        off[1:] = torch.cumsum(ln, 0)
        pos = torch.arange(int(off[-1].item()), device=self.device) - torch.repeat_interleave(off[:-1] - beg, ln)
        return off.int(), self._some_ids(ids[pos].contiguous())

    def _topk_from_rows(self, score_rows, n, k, return_scores):
        """Explicit score rows, a bounded number at a time, + poi_topk (k <= 64).  score_rows(o, c) -> (c, n_item) float32 scores of
        rows o .. o + c - 1."""
        k = int(k)
        if k > 64:
            raise _lib.PoiError("top-K supports k <= 64 (got %d)" % k)
        idx, sc, _ = self._topk_buffers(n, k, return_scores, False)
        for o, c in self._row_chunks(n):
            full = score_rows(o, c)
            self.ctx.check(self.lib.poi_topk(self.ctx.handle, _ptr(full), full.shape[0], self.n_item, k, _at(idx, o, k), _at(sc, o, k), self._stream()))
        return (idx, sc) if return_scores else idx

    def _topk_from_scores(self, start_end, k, return_scores=False, scores=None):
        """Cut-offs beyond the fused kernels' k <= 32 (e.g. at_nums = [5, 10, 15, 20, 30, 50], public/Valuate.py:126): the rows of
        compute_sub_all_scores_device (or `scores`) through _topk_from_rows."""
        a = self._id_list(start_end)
        rows = scores or self.compute_sub_all_scores_device
        return self._topk_from_rows(lambda o, c: rows(a[o:o + c]), len(a), k, return_scores)


    # ---- restricted recommendation (poi_score_topk_near): top-K within a radius of an anchor POI, skipping listed POIs -----------------
    _near_ok = True         # False: the model ranks by a score rule of its own (CA-RNN, PRME, GeoIE, POI2Vec)

    def set_coords(self, coords):
        """POI coordinates ((n_item, 2) lat, lon) for a model constructed without them (the MfBasic family, plain GruBasic): uploads
        coords, cos(lat) (data.cos_lat) and the stable latitude order that the radius test of compute_sub_topk_near / Session.recommend
        walks.  Models that were given coords= at construction need no call: they build the latitude order at first use."""
        xy = np.ascontiguousarray(coords.cpu().numpy() if isinstance(coords, torch.Tensor) else coords, np.float64)
        if xy.shape != (self.n_item, 2):
            raise ValueError("coords must be (n_item, 2) lat, lon (got %s)" % (xy.shape,))
        self.coords = torch.as_tensor(xy).to(self.device)
        self._cphi = torch.as_tensor(cos_lat(xy)).to(self.device)
        self._lat_order = None
        if getattr(self, "spatial", False):
            self._binthr = self._dev(bin_thresholds(self.dd * 1000.0, self.n_dist), torch.float64)

    def _near_geo(self, radius):
        """(coords, cphi, lat_order | None) on the device; the order is built once."""
        if getattr(self, "coords", None) is None:
            raise _lib.PoiError("%s holds no POI coordinates: call set_coords(coords) first" % type(self).__name__)
        if radius and getattr(self, "_lat_order", None) is None:
            self._lat_order = torch.argsort(self.coords[:, 0], stable=True).to(torch.int32).contiguous()
        return self.coords, self._cphi, (self._lat_order if radius else None)

    def _near_radius(self, within_km):
        """within_km -> the Haversine threshold c_r (data.ud_threshold; None / inf: no radius test)."""
        from .data import ud_threshold
        if within_km is None:
            return float("inf")
        r = float(within_km)
        if not r >= 0.0:
            raise ValueError("within_km must be >= 0 (got %r)" % (within_km,))
        cache = self.__dict__.setdefault("_near_thr", {})
        if r not in cache:
            cache[r] = float(ud_threshold(r))
        return cache[r]

    def _near_items(self):
        return self._items()

    def _near_term(self, ids, lo):
        """(wd, sts rows (n, n_dist + 1), thr, n_dist, dd in metres) of the model's distance term, or None."""
        return None

    def _last_train_poi(self):
        """(n_user) int32 device: every user's last train POI (-1 for an empty train row)."""
        t = self.__dict__.get("_near_last")
        if t is None:
            off = self._off_host.astype(np.int64)
            t = self.p.index_select(0, torch.as_tensor(np.maximum(off[1:] - 1, 0)).to(self.device)).clone()
            t[torch.as_tensor(off[1:] == off[:-1]).to(self.device)] = -1
            self._near_last = t
        return t

    def train_exclusion(self):
        """Every user's DISTINCT train POIs as a sorted CSR (off (n_user + 1) int32, ids int32) on the device - built once (the train
        tables do not change) and cached: the exclude="train" lists."""
        t = self.__dict__.get("_near_train")
        if t is None:
            from .data import train_exclusion_csr
            eo, key = train_exclusion_csr(self._off_host, self.p.cpu().numpy(), self.n_item)
            i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
            t = self._near_train = (i32(eo), i32(key))
        return t

    def _near_exclusion(self, exclude, n, anchor, ids=None, lo=None, kinds=("train", "last")):
        """exclude -> (ex_off (n + 1), ex) int32 device tensors, or (None, None)."""
        if exclude is None:
            return None, None
        if isinstance(exclude, str):
            if exclude not in kinds:
                raise ValueError("exclude must be None, %s or a pair (off, ids) (got %r)" % (", ".join(repr(k) for k in kinds), exclude))
            if exclude == "last":                               # the anchor alone (a row without one excludes nothing)
                has = (anchor >= 0)
                eo = torch.zeros(n + 1, dtype=torch.int32, device=self.device)
                eo[1:] = torch.cumsum(has.int(), 0)
                return eo, self._some_ids(anchor[has].contiguous())
            eo, ex = self.train_exclusion()
            if lo is not None:                                  # a contiguous user range: its offsets index the cached ids as they are
                return eo[lo:lo + n + 1], ex
            u = ids.long()
            return self._csr_take(ex, eo[u].long(), (eo[u + 1] - eo[u]).long())
        off, lst = exclude
        if isinstance(off, torch.Tensor) and isinstance(lst, torch.Tensor):      # device lists are checked by the kernel
            if off.numel() != n + 1:
                raise ValueError("exclude=(off, ids): off must hold n + 1 = %d offsets" % (n + 1))
            return off.to(self.device, torch.int32).contiguous(), self._some_ids(lst.to(self.device, torch.int32).contiguous())
        off = off.cpu().numpy() if isinstance(off, torch.Tensor) else off
        lst = lst.cpu().numpy() if isinstance(lst, torch.Tensor) else lst
        from .data import check_exclusion_csr
        eo, ex = (torch.as_tensor(v).to(self.device) for v in check_exclusion_csr(off, lst, n, self.n_item))
        return eo, self._some_ids(ex)

    def _tile_operands(self, users, items, kdim, term):
        """The 13 arguments that follow the context handle in poi_score_rank / poi_group_topk / poi_route_expand / poi_diverse_topk
        (users .. dd).  term: (wd, sts rows, last POI rows) of the model's distance term, or None."""
        wd = sts = lp = coords = cphi = thr = None
        n_dist, dd_m = 0, 0.0
        if term is not None:
            wd, sts, lp = term
            coords, cphi, thr, n_dist, dd_m = self.coords, self._cphi, self._binthr, self.n_dist, self.dd * 1000.0
        return [_ptr(users), _ptr(items), users.shape[0], self.n_item, kdim, _ptr(wd), _ptr(sts), _ptr(coords), _ptr(cphi), _ptr(thr), _ptr(lp),
                int(n_dist), float(dd_m)]

    def _serve_out(self, first, optional_pairs, sync, message):
        """What a serving call returns: `first`, then every (tensor, wanted) pair that is wanted; alone, `first` itself.  With sync the
        kernels' count of rejected rows is read first and raises IndexError("<count> <message>")."""
        if sync:
            bad = self.ctx.take_bad_ids(self._stream().value)
            if bad:
                raise IndexError("%d %s" % (bad, message))
        out = (first,) + tuple(t for t, wanted in optional_pairs if wanted)
        return out if len(out) > 1 else first

    def _near_launch(self, users, items, anchor, c_r, ex, term, k, return_scores, return_counts, sync):
        """One poi_score_topk_near call -> idx[, scores][, counts] (device tensors)."""
        n, k = users.shape[0], int(k)
        radius = c_r < float("inf")
        coords = cphi = order = None
        if radius or term is not None:
            coords, cphi, order = self._near_geo(radius)
        wd, sts, thr, n_dist, dd_m = term if term is not None else (None, None, None, 0, 0.0)
        idx, sc, cnt = self._topk_buffers(n, max(k, 0), return_scores, return_counts)
        self.ctx.check(self.lib.poi_score_topk_near(self.ctx.handle, _ptr(users), _ptr(items), n, self.n_item, self.kdim, _ptr(coords), _ptr(cphi),
                                                    _ptr(order), _ptr(anchor), c_r, _ptr(ex[0]), _ptr(ex[1]), _ptr(wd), _ptr(sts), _ptr(thr),
                                                    int(n_dist), float(dd_m), k, _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync,
                               "row(s) with an anchor outside [-1, %d) or an exclusion id outside [0, %d): their lists are all -1" % (self.n_item, self.n_item))

    def _near_anchor(self, anchor, n, default):
        """anchor argument -> (n) int32 device tensor; host arrays are range-checked ([-1, n_item), -1 = no anchor) before any launch."""
        if anchor is None:
            return default()
        if isinstance(anchor, torch.Tensor):
            t = anchor.to(self.device, torch.int32).contiguous().reshape(-1)
        else:
            a = np.atleast_1d(np.asarray(anchor)).astype(np.int64)
            if a.size and (a.min() < -1 or a.max() >= self.n_item):
                raise IndexError("anchor ids must lie in [-1, %d) (found %d..%d)" % (self.n_item, int(a.min()), int(a.max())))
            t = torch.as_tensor(a.astype(np.int32)).to(self.device)
        if t.numel() != n:
            raise ValueError("anchor must hold one POI per row (%d vs %d)" % (t.numel(), n))
        return t

    def compute_sub_topk_near(self, start_end, k, within_km=None, exclude=None, anchor=None, return_scores=False, return_counts=False, sync=True):
        """compute_sub_topk over RESTRICTED candidates (include/poi_hip.h, poi_score_topk_near): the POIs within `within_km` km of the
        row's anchor (cal_dis <= within_km, exactly; None: no radius; default anchor: the user's last train POI; anchor -1: no radius
        for that row), minus the row's exclusion list - None, "train" (the user's distinct train POIs), "last" (the anchor) or a pair
        (off, ids) of CSR lists, ids ascending and unique per row.  Returns (n, k) int32 ids by descending score (k <= 32), ties by
        ascending id, -1 where a row has fewer than k candidates (scores -inf); with return_counts the candidate count of every row.
        The score is the model's own: users . items at kdim, plus the spatial model's distance term taken at the anchor.  With
        within_km=None and exclude=None this is compute_sub_topk.  Host arguments are checked before the launch; device tensors are
        checked by the kernel: an offending row comes out all -1 and - with sync - raises IndexError (sync=False leaves the count to
        ctx.take_bad_ids())."""
        if not self._near_ok:                                    # (before anything of the model is read)
            raise _lib.PoiError(self._refusals()["near"])
        if within_km is None and exclude is None and anchor is None:
            out = self.compute_sub_topk(start_end, k, return_scores)
            if return_counts:
                n = (out[0] if return_scores else out).shape[0]
                cnt = torch.full((n,), self.n_item, dtype=torch.int32, device=self.device)
                out = (out + (cnt,)) if return_scores else (out, cnt)
            return out
        return self._serve_near(self._source(start_end, ("train", "last"), True), k, within_km, exclude, anchor, return_scores, return_counts, sync)

    def _serve_near(self, src, k, within_km, exclude, anchor, return_scores, return_counts, sync):
        """The restricted top-K of a source's rows: anchor (default the source's), exclusion lists, one poi_score_topk_near call."""
        src.need_fused("near")
        anc = self._near_anchor(anchor, src.n, src.anchor)
        ex = src.exclusion(exclude, anc)
        return self._near_launch(src.users, src.items, anc, self._near_radius(within_km), ex, src.near_term(), k, return_scores, return_counts, sync)

    # ---- exact target ranks (poi_score_rank / poi_rank_scores): where the held-out POIs stand among ALL POIs ---------------------------
    _rank_fused = True      # False: the model's score is not users . items - explicit score rows + poi_rank_scores

    def _rank_term(self, ids, lo):
        """(wd, sts rows (n, n_dist + 1), last POI rows (n)) of the model's distance term, or None."""
        return None

    def _rank_targets(self, targets, n):
        """targets -> (tgt, tmask) int32 device tensors (n, len_t): an (n, len_t) array of POI ids (all valid), or a pair (ids, mask)."""
        tgt, tm = targets if isinstance(targets, tuple) and len(targets) == 2 else (targets, None)
        rows = lambda t: t if t.dim() == 2 and t.shape[0] == n else t.reshape(n, -1)      # ((0, len_t) rows cannot be reshaped)
        tgt = rows(self._dev(tgt, torch.int32))
        tm = torch.ones_like(tgt) if tm is None else rows(self._dev(tm, torch.int32))
        if tgt.shape != tm.shape:
            raise ValueError("targets and their mask must have the same shape (%s vs %s)" % (tuple(tgt.shape), tuple(tm.shape)))
        if not 1 <= tgt.shape[1] <= 8:
            raise _lib.PoiError("target ranks support 1 .. 8 targets per row (got %d)" % tgt.shape[1])
        return tgt.contiguous(), tm.contiguous()

    def _rank_out(self, rank, sc, cnt, return_scores, return_counts, sync):
        return self._serve_out(rank, ((sc, return_scores), (cnt, return_counts)), sync,
                               "target(s) outside [0, %d) or row(s) with a malformed exclusion list: their ranks are -1" % self.n_item)

    def _rank_launch(self, users, items, term, tgt, tm, ex, return_scores, return_counts, sync):
        """One poi_score_rank call -> rank[, scores][, counts] (device tensors)."""
        n, lt = users.shape[0], tgt.shape[1]
        rank, sc, cnt = self._topk_buffers(n, lt, return_scores, return_counts)
        self.ctx.check(self.lib.poi_score_rank(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(tgt), _ptr(tm), lt,
                                               _ptr(ex[0]), _ptr(ex[1]), _ptr(rank), _ptr(sc), _ptr(cnt), self._stream()))
        return self._rank_out(rank, sc, cnt, return_scores, return_counts, sync)

    def _rank_score_rows(self, a):
        """Fallback models: (score rows (m, n_item) ranked by descending value, rows per user) for the users `a`."""
        return self.compute_sub_all_scores_device(a), 1

    def _rank_from_scores(self, score_rows, n, tgt, tm, ex, return_scores, return_counts, sync, step=None):
        """Explicit score rows, a bounded number of rows at a time (`step`: not the model's _rank_chunk), + poi_rank_scores.
        score_rows(o, c) -> (c, n_item) float32 scores of rows o .. o + c - 1, or (c * per, n_item) rows (row, position), row-major."""
        lt = tgt.shape[1]
        rank, sc, cnt = self._topk_buffers(n, lt, return_scores, return_counts)
        for o, c in self._row_chunks(n, step):
            full = score_rows(o, c)
            per = full.shape[0] // c
            t_c, m_c = tgt[o:o + c], tm[o:o + c]
            eo = ex[0][o:o + c + 1].contiguous() if ex[0] is not None else None
            if per == 1:
                r_c = torch.empty((c, lt), dtype=torch.int32, device=self.device)
                k_c = torch.empty(c, dtype=torch.int32, device=self.device) if cnt is not None else None
                self.ctx.check(self.lib.poi_rank_scores(self.ctx.handle, _ptr(full), c, self.n_item, _ptr(t_c.contiguous()), _ptr(m_c.contiguous()), lt,
                                                        _ptr(eo), _ptr(ex[1]), _ptr(r_c), _ptr(k_c), self._stream()))
            else:
                # rows (user, position): position t ranks the user's t-th target; positions beyond `per` stay -1
                w = min(per, lt)
                t_r = torch.zeros((c, per), dtype=torch.int32, device=self.device); m_r = torch.zeros_like(t_r)
                t_r[:, :w] = t_c[:, :w]; m_r[:, :w] = m_c[:, :w]
                if eo is not None:                               # every position of a user shares the user's list
                    e_r = self._csr_take(ex[1], eo[:-1].long().repeat_interleave(per), (eo[1:] - eo[:-1]).long().repeat_interleave(per))
                else:
                    e_r = (None, None)
                r_r = torch.empty((c * per, 1), dtype=torch.int32, device=self.device)
                k_r = torch.empty(c * per, dtype=torch.int32, device=self.device) if cnt is not None else None
                self.ctx.check(self.lib.poi_rank_scores(self.ctx.handle, _ptr(full), c * per, self.n_item, _ptr(t_r.reshape(-1, 1)), _ptr(m_r.reshape(-1, 1)), 1,
                                                        _ptr(e_r[0]), _ptr(e_r[1]), _ptr(r_r), _ptr(k_r), self._stream()))
                r_c = torch.full((c, lt), -1, dtype=torch.int32, device=self.device)
                r_c[:, :w] = r_r.view(c, per)[:, :w]
                k_c = k_r.view(c, per)[:, 0] if k_r is not None else None
                full = full.view(c, per, self.n_item)
            rank[o:o + c] = r_c
            if cnt is not None:
                cnt[o:o + c] = k_c
            if sc is not None:
                ok = r_c >= 0
                g = t_c.long().clamp(0, self.n_item - 1)
                if per == 1:
                    v = full.gather(1, g)
                else:
                    w = min(per, lt)
                    v = torch.full((c, lt), float("-inf"), dtype=torch.float32, device=self.device)
                    v[:, :w] = full[:, :w].gather(2, g[:, :w, None])[:, :, 0]
                sc[o:o + c] = torch.where(ok, v, torch.full_like(v, float("-inf")))
        return self._rank_out(rank, sc, cnt, return_scores, return_counts, sync)

    def compute_sub_target_rank(self, start_end, exclude=None, targets=None, return_scores=False, return_counts=False, sync=True):
        """Exact 0-based rank of each target POI among ALL POIs under the model's own score (include/poi_hip.h, poi_score_rank): the
        number of POIs with a higher score, or an equal score and a lower id - the position the target would have in an endless
        compute_sub_topk list.  targets: None = the rows' test POIs (tes_buys_masks / tes_masks), an (n, len_t <= 8) array of POI ids, or
        a pair (ids, mask).  exclude: None, "train" (the user's distinct train POIs leave the ranking) or CSR lists (off, ids), as
        compute_sub_topk_near.  Returns (n, len_t) int32 on the device, -1 for a masked position, an excluded target or a target outside
        [0, n_item) (which - with sync - raises IndexError); with return_scores the targets' scores, with return_counts the number of
        ranked POIs per row.  No (n, n_item) matrix is built for the models that score by users . items; CA-RNN, PRME and POI2Vec go
        through their own score rows, a bounded number of users at a time, and poi_rank_scores."""
        src = self._source(start_end)
        if targets is None:
            targets = self._rows(self.tes_buys_masks, src.ids, src.lo), self._rows(self.tes_masks, src.ids, src.lo)
        return self._serve_rank(src, targets, exclude, return_scores, return_counts, sync)

    def _serve_rank(self, src, targets, exclude, return_scores, return_counts, sync):
        """The exact ranks of a source's rows: poi_score_rank on the last POI rows clamped to 0, or every (row, position) score row +
        poi_rank_scores."""
        tgt, tm = self._rank_targets(targets, src.n)
        ex = src.exclusion(exclude)
        if src.fused:
            out = self._rank_launch(src.users, src.items, src.tile_term(clamp=True), tgt, tm, ex, return_scores, return_counts, sync)
        else:
            out = self._rank_from_scores(src.score_rows(positions=True), src.n, tgt, tm, ex, return_scores, return_counts, sync)
        return src.finish(out, return_scores, return_counts, ranked=True)


    # ---- candidate generation (poi_score_candidates / poi_topk_select): the exact top-K of every row for K up to 4096 ----------------------
    CANDIDATES_K_MAX = 4096

    def _candidates_k(self, k):
        k = int(k)
        if not 1 <= k <= min(self.CANDIDATES_K_MAX, self.n_item):
            raise ValueError("candidate generation supports 1 <= k <= min(%d, n_item = %d) (got %d)" % (self.CANDIDATES_K_MAX, self.n_item, k))
        return k

    def _candidates_out(self, idx, sc, cnt, return_scores, return_counts, sync):
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync,
                               "row(s) with a malformed exclusion list: their candidate lists are all -1")

    def _candidates_launch(self, users, items, term, ex, k, return_scores, return_counts, sync):
        """One poi_score_candidates call -> idx[, scores][, counts] (device tensors).  term: (wd, sts rows, last POI rows) or None."""
        n = users.shape[0]
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        if n:
            self.ctx.check(self.lib.poi_score_candidates(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), k, _ptr(ex[0]), _ptr(ex[1]),
                                                         _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        return self._candidates_out(idx, sc, cnt, return_scores, return_counts, sync and n > 0)

    def _candidates_from_scores(self, score_rows, n, ex, k, return_scores, return_counts, sync):
        """Explicit score rows, a bounded number of rows at a time, + poi_topk_select, which takes the exclusion lists itself (the rows
        are not masked on the host).  score_rows(o, c) -> (c, n_item) float32 scores of rows o .. o + c - 1."""
        N = self.n_item
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        for o, c in self._row_chunks(n):
            full = score_rows(o, c).contiguous()
            self.ctx.check(self.lib.poi_topk_select(self.ctx.handle, _ptr(full), c, N, N, k, _at(ex[0], o, 1), _ptr(ex[1]), _at(idx, o, k), _at(sc, o, k),
                                                    _at(cnt, o, 1), self._stream()))
        return self._candidates_out(idx, sc, cnt, return_scores, return_counts, sync and n > 0)

    def compute_sub_candidates(self, start_end, k, exclude=None, return_scores=False, return_counts=False, sync=True):
        """CANDIDATE GENERATION (include/poi_hip.h, poi_score_candidates): the exact top-k of every row under the model's own score for
        1 <= k <= min(4096, n_item) - the hand-over of a retrieval stage to a downstream ranker, where compute_sub_topk stops at a short
        list.  exclude: None, "train" (the user's distinct train POIs) or CSR lists (off, ids), ids ascending and unique per row.
        Returns (n, k) int32 ids on the device by descending score, ties by ascending id (-0.0 and +0.0 are one score), -1 where a row
        has fewer than k selectable POIs (NaN and -inf scores are never selected; scores -inf); with return_scores the scores, with
        return_counts the candidate count of every row.  The models that score by users . items make one fused call (the score rows
        live in a bounded workspace of the context, option "select_chunk_mb"); CA-RNN, PRME, POI2Vec and GeoIE under rule="geo" go
        through their own score rows, a bounded number at a time, and poi_topk_select.  Host arguments are checked before the launch
        (ValueError / IndexError); device lists are checked by the kernel: an offending row comes out all -1 and - with sync - raises
        IndexError."""
        return self._serve_candidates(self._source(start_end), k, exclude, return_scores, return_counts, sync)

    def _serve_candidates(self, src, k, exclude, return_scores, return_counts, sync):
        """The exact top-k <= 4096 of a source's rows: poi_score_candidates, or its score rows + poi_topk_select."""
        k = self._candidates_k(k)
        ex = src.exclusion(exclude)
        if src.fused:
            out = self._candidates_launch(src.users, src.items, src.tile_term(), ex, k, return_scores, return_counts, sync)
        else:
            out = self._candidates_from_scores(src.score_rows(), src.n, ex, k, return_scores, return_counts, sync)
        return src.finish(out, return_scores, return_counts)


    # ---- re-ranking (poi_score_lists / poi_rerank_lists / poi_rerank): score explicit candidate lists, blend with a prior, exact top-K -----
    RERANK_LEN_MAX = 4096
    _RERANK_MESSAGE = ("row(s) with malformed candidate offsets, more than %d candidates or a candidate id beyond the table: "
                       "their scores are -inf, their lists all -1" % RERANK_LEN_MAX)

    def _rerank_lists_arg(self, lists, n, host_check=False):
        """lists -> dict(off, ids (device int32; off None = one shared list), n_cand, shape): an (n, C) array or tensor padded with -1
        (shape (n, C): a ragged list with off[r] = r C), a CSR pair (off, ids) (shape None: flat) or a 1-D array, one list shared by
        every row (shape (n, C)).  Host arrays are checked before the launch - offsets ascending inside the ids (ValueError), ids below
        n_item (IndexError; negative ids are padding); device tensors are left to the kernel, unless `host_check` copies them back."""
        def host(a):
            if isinstance(a, torch.Tensor):
                return a.cpu().numpy() if host_check or not a.is_cuda else None
            return np.asarray(a)

        def ids_dev(a, h):
            if h is not None:
                h = np.ascontiguousarray(h).reshape(-1).astype(np.int64)
                if h.size and h.max() >= self.n_item:
                    raise IndexError("candidate ids must lie below n_item = %d (found %d); negative ids are padding" % (self.n_item, int(h.max())))
                t = torch.as_tensor(h.astype(np.int32)).to(self.device)
            else:
                t = a.to(self.device, torch.int32).contiguous().reshape(-1)
            return self._some_ids(t)

        if isinstance(lists, tuple):
            if len(lists) != 2:
                raise ValueError("lists=(off, ids): a CSR pair")
            off, ids = lists
            n_cand = int(ids.numel() if isinstance(ids, torch.Tensor) else np.asarray(ids).size)
            if (off.numel() if isinstance(off, torch.Tensor) else np.asarray(off).size) != n + 1:
                raise ValueError("lists=(off, ids): off must hold n + 1 = %d offsets" % (n + 1))
            ho = host(off)
            if ho is not None:
                ho = ho.reshape(-1).astype(np.int64)
                if ho[0] < 0 or np.any(np.diff(ho) < 0) or ho[-1] > n_cand:
                    raise ValueError("lists=(off, ids): the offsets must ascend inside [0, %d]" % n_cand)
                off_t = torch.as_tensor(ho.astype(np.int32)).to(self.device)
            else:
                off_t = off.to(self.device, torch.int32).contiguous().reshape(-1)
            return dict(off=off_t, ids=ids_dev(ids, host(ids)), n_cand=n_cand, shape=None, host_off=ho)
        h = host(lists)
        shape = tuple(lists.shape) if isinstance(lists, torch.Tensor) else h.shape
        if len(shape) == 1:
            return dict(off=None, ids=ids_dev(lists, h), n_cand=int(shape[0]), shape=(n, int(shape[0])), host_off=None)
        if len(shape) != 2 or shape[0] != n:
            raise ValueError("lists must be (n = %d, C) padded with -1, a CSR pair (off, ids) or one 1-D shared list (got shape %s)" % (n, shape))
        C = int(shape[1])
        ho = np.arange(n + 1, dtype=np.int64) * C
        if ho[-1] >= 2 ** 31:
            raise ValueError("lists: n * C must stay below 2^31")
        off_t = torch.arange(n + 1, dtype=torch.int32, device=self.device) * C      # (built on the device: no copy in front of the launch)
        return dict(off=off_t, ids=ids_dev(lists, h), n_cand=n * C, shape=(n, C), host_off=ho)

    def _rerank_args(self, L, n, k, prior, weights):
        """k, the prior as a device float32 tensor laid out like the scores (or None), the two weights."""
        k = int(k)
        if not 1 <= k <= self.RERANK_LEN_MAX:
            raise ValueError("re-ranking supports 1 <= k <= %d (got %d)" % (self.RERANK_LEN_MAX, k))
        longest = L["n_cand"] if L["off"] is None else L["shape"][1] if L["shape"] else int(np.diff(L["host_off"]).max()) if L["host_off"] is not None and n else 0
        if longest > self.RERANK_LEN_MAX:
            raise ValueError("re-ranking supports lists of at most %d candidates (got %d)" % (self.RERANK_LEN_MAX, longest))
        w = tuple(float(x) for x in weights)
        if len(w) != 2:
            raise ValueError("weights = (w_score, w_prior)")
        if prior is not None:
            prior = self._dev(prior, torch.float32).reshape(-1)
            want = L["n_cand"] if L["off"] is not None else n * L["n_cand"]
            if prior.numel() != want:
                raise ValueError("prior must hold one value per candidate entry (%d vs %d)" % (prior.numel(), want))
            if not prior.numel():
                prior = torch.zeros(1, dtype=torch.float32, device=self.device)
        return k, prior, w

    def _rerank_buffers(self, n, k, return_scores, return_positions, return_counts):
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        return idx, sc, (torch.empty((n, k), dtype=torch.int32, device=self.device) if return_positions else None), cnt

    def _lists_scores_buffer(self, L, n):
        numel = L["n_cand"] if L["off"] is not None else n * L["n_cand"]
        return torch.empty(max(numel, 1), dtype=torch.float32, device=self.device), numel

    def _lists_scores_out(self, buf, numel, L):
        out = buf[:numel]
        return out.view(L["shape"]) if L["shape"] is not None else out

    def _score_lists_launch(self, users, items, term, L, sync):
        """One poi_score_lists call -> the scores, laid out like the lists."""
        n = users.shape[0]
        buf, numel = self._lists_scores_buffer(L, n)
        if n and numel:
            self.ctx.check(self.lib.poi_score_lists(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(L["off"]), _ptr(L["ids"]),
                                                    L["n_cand"], _ptr(buf), self._stream()))
        return self._serve_out(self._lists_scores_out(buf, numel, L), (), sync and n > 0 and numel > 0, self._RERANK_MESSAGE)

    def _rerank_launch(self, users, items, term, L, k, prior, w, return_scores, return_positions, return_counts, sync):
        """One poi_rerank call -> idx[, keys][, positions][, counts] (device tensors)."""
        n = users.shape[0]
        idx, sc, pos, cnt = self._rerank_buffers(n, k, return_scores, return_positions, return_counts)
        if n:
            self.ctx.check(self.lib.poi_rerank(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(L["off"]), _ptr(L["ids"]),
                                               L["n_cand"], _ptr(prior), w[0], w[1], k, _ptr(idx), _ptr(sc), _ptr(pos), _ptr(cnt), self._stream()))
        return self._serve_out(idx, ((sc, return_scores), (pos, return_positions), (cnt, return_counts)), sync and n > 0, self._RERANK_MESSAGE)

    def _lists_from_rows(self, score_rows, n, L):
        """The listed columns of explicit score rows, a bounded number of rows at a time (score_rows(o, c) -> (c, n_item)): a torch
        gather.  The lists have been checked on the host (_rerank_lists_arg(host_check=True)); padding gets -inf."""
        buf, numel = self._lists_scores_buffer(L, n)
        ids = L["ids"][:L["n_cand"]].long()
        col, pad = ids.clamp(min=0), ids < 0
        for o, c in self._row_chunks(n):
            full = score_rows(o, c)
            if L["off"] is None:
                part = full.index_select(1, col).masked_fill(pad[None, :], float("-inf"))
                buf[o * L["n_cand"]:(o + c) * L["n_cand"]] = part.reshape(-1)
            else:
                e0, e1 = int(L["host_off"][o]), int(L["host_off"][o + c])
                lens = torch.as_tensor(np.diff(L["host_off"][o:o + c + 1])).to(self.device)
                row = torch.repeat_interleave(torch.arange(c, device=self.device), lens)
                buf[e0:e1] = full[row, col[e0:e1]].masked_fill(pad[e0:e1], float("-inf"))
        if L["off"] is not None and numel:                       # entries no row owns
            own = torch.zeros(numel, dtype=torch.bool, device=self.device)
            own[int(L["host_off"][0]):int(L["host_off"][-1])] = True
            buf[:numel].masked_fill_(~own, float("-inf"))
        return buf, numel

    def _rerank_from_scores(self, score_rows, n, L, k, prior, w, return_scores, return_positions, return_counts, sync):
        """Explicit score rows + a gather of the listed columns + poi_rerank_lists."""
        idx, sc, pos, cnt = self._rerank_buffers(n, k, return_scores, return_positions, return_counts)
        if n:
            buf, _ = self._lists_from_rows(score_rows, n, L)
            self.ctx.check(self.lib.poi_rerank_lists(self.ctx.handle, _ptr(L["off"]), _ptr(L["ids"]), n, L["n_cand"], _ptr(buf), _ptr(prior), w[0], w[1], k,
                                                     _ptr(idx), _ptr(sc), _ptr(pos), _ptr(cnt), self._stream()))
        return self._serve_out(idx, ((sc, return_scores), (pos, return_positions), (cnt, return_counts)), sync and n > 0, self._RERANK_MESSAGE)

    def score_lists(self, start_end, lists, sync=True):
        """The model's own score of EXPLICIT candidates (include/poi_hip.h, poi_score_lists): `lists` is an (n, C) array or tensor
        padded with -1, a CSR pair (off, ids) or a 1-D array - one list shared by every row.  Returns float32 scores on the device
        laid out like the lists ((n, C), flat, (n, C)); padding gets -inf.  The scores are compute_sub_all_scores' at the listed
        columns - for the models that score by users . items bit for bit poi_score_rows', without the (n, n_item) matrix."""
        return self._serve_score_lists(self._source(start_end), lists, sync)

    def _serve_score_lists(self, src, lists, sync):
        """The scores of explicit candidate lists under a source's rows: poi_score_lists, or the listed columns of its score rows (the
        lists then checked on the host, device lists too)."""
        L = self._rerank_lists_arg(lists, src.n, host_check=not src.fused)
        if src.fused:
            return self._score_lists_launch(src.users, src.items, src.tile_term(), L, sync)
        buf, numel = self._lists_from_rows(src.score_rows(), src.n, L) if src.n else self._lists_scores_buffer(L, 0)
        return self._lists_scores_out(buf, numel, L)

    def rerank(self, start_end, lists, k, prior=None, weights=(1.0, 0.0), return_scores=False, return_positions=False, return_counts=False,
               sync=True):
        """RE-RANKING (include/poi_hip.h, poi_rerank): the second stage of a two-stage recommender.  Every row brings its candidate POIs
        (`lists`, as score_lists takes them: e.g. another model's compute_sub_candidates output); they are scored under THIS model and
        the best k <= 4096 come back in order.  With a prior (one float per candidate entry, laid out like the lists) the key is
        weights[0] * score + weights[1] * prior in float64, rounded once to float32; without one the key is the score.  Returns (n, k)
        int32 ids on the device by descending key, ties by ascending id, then by position in the list (duplicates are kept), -1
        where a list has fewer than k selectable entries (padding, NaN and -inf keys are never selected); with return_scores the keys,
        with return_positions each entry's position inside its list (gather side data with it), with return_counts the number of
        selectable entries per row.  The models that score by users . items make one fused call; CA-RNN, PRME, POI2Vec and GeoIE under
        rule="geo" go through their own score rows, a bounded number at a time, a gather and poi_rerank_lists.  Host arguments are
        checked before the launch (ValueError / IndexError); device lists are checked by the kernel: an offending row comes out all
        -1 and - with sync - raises IndexError."""
        return self._serve_rerank(self._source(start_end), lists, k, prior, weights, return_scores, return_positions, return_counts, sync)

    def _serve_rerank(self, src, lists, k, prior, weights, return_scores, return_positions, return_counts, sync):
        """A source's rows re-rank their candidate lists: poi_rerank, or the listed columns of its score rows + poi_rerank_lists."""
        L = self._rerank_lists_arg(lists, src.n, host_check=not src.fused)
        k, prior, w = self._rerank_args(L, src.n, k, prior, weights)
        if src.fused:
            return self._rerank_launch(src.users, src.items, src.tile_term(), L, k, prior, w, return_scores, return_positions, return_counts, sync)
        return self._rerank_from_scores(src.score_rows(), src.n, L, k, prior, w, return_scores, return_positions, return_counts, sync)


    # ---- filtered recommendation (poi_filter_build / poi_score_topk_filtered / poi_topk_filtered_scores): top-K among the POIs that pass a predicate
    FILTER_K_MAX = 32
    _FILTER_PATH = {"auto": 0, "walk": 1, "gather": 2}

    def set_attributes(self, categories=None, flags=None, n_cat=None):
        """POI attributes for poi_filter - the caller's, as VBPR's feature table and set_coords are (the reference data has none).
        categories: (n_item) ints in [0, n_cat), n_cat <= 4096 (default: the largest category + 1); flags: (n_item) uint32 words whose
        bits mean what the application says (price tier, open now, ...).  Either may be None."""
        cat = fl = None
        if categories is not None:
            c = categories.cpu().numpy() if isinstance(categories, torch.Tensor) else np.asarray(categories)
            if c.shape != (self.n_item,):
                raise ValueError("categories must hold one id per POI (%s vs n_item = %d)" % (c.shape, self.n_item))
            n_cat = int(c.max()) + 1 if n_cat is None else int(n_cat)
            cat = torch.as_tensor(np.ascontiguousarray(c, dtype=np.int32)).to(self.device)
        n_cat = 1 if n_cat is None else int(n_cat)
        if not 1 <= n_cat <= 4096:
            raise ValueError("n_cat must lie in [1, 4096] (got %d)" % n_cat)
        if flags is not None:
            f = flags.cpu().numpy() if isinstance(flags, torch.Tensor) else np.asarray(flags)
            if f.shape != (self.n_item,):
                raise ValueError("flags must hold one word per POI (%s vs n_item = %d)" % (f.shape, self.n_item))
            fl = torch.as_tensor(np.ascontiguousarray(f.astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).view(np.int32)).to(self.device)
        self._attr = (cat, fl, n_cat)

    def poi_filter(self, predicates):
        """predicates: a list of dicts with any of "categories" (ids; absent or empty: any category), "need" (flag bits that must all
        be set), "any" (at least one of them set; 0: no condition) and "forbid" (none of them set) -> a PoiFilter over the model's
        attributes (set_attributes).  One kernel and one synchronisation (the counts come to the host): a set-up step, like
        set_coords.  A POI whose category lies outside [0, n_cat) passes no predicate with a category list and raises IndexError."""
        cat, fl, n_cat = self.__dict__.get("_attr", (None, None, 1))
        preds = list(predicates)
        if not preds:
            raise ValueError("poi_filter needs at least one predicate")
        off, pcs, words = [0], [], []
        for q, d in enumerate(preds):
            extra = set(d) - {"categories", "need", "any", "forbid"}
            if extra:
                raise ValueError("predicate %d: unknown key(s) %s" % (q, sorted(extra)))
            c = np.unique(np.asarray(list(d.get("categories") or ()), np.int64))
            if c.size:
                if cat is None:
                    raise _lib.PoiError("predicate %d lists categories but the model holds none: call set_attributes(categories=...)" % q)
                if c.min() < 0 or c.max() >= n_cat:
                    raise ValueError("predicate %d: category ids must lie in [0, %d)" % (q, n_cat))
            pcs.append(c); off.append(off[-1] + c.size)
            w = [int(d.get(key, 0)) for key in ("need", "any", "forbid")]
            if any(not 0 <= v <= 0xFFFFFFFF for v in w):
                raise ValueError("predicate %d: need / any / forbid are 32-bit words" % q)
            words.append(w)
        P, W = len(preds), (self.n_item + 31) // 32
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        u32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.device)
        pc = np.concatenate(pcs) if off[-1] else np.zeros(1, np.int64)
        wd = np.asarray(words, np.uint32)
        t_off, t_pc, t_need, t_any, t_forbid = i32(off), i32(pc), u32(wd[:, 0]), u32(wd[:, 1]), u32(wd[:, 2])
        bits = torch.empty((P, W), dtype=torch.int32, device=self.device)
        cnt = torch.empty(P, dtype=torch.int32, device=self.device)
        self.ctx.check(self.lib.poi_filter_build(self.ctx.handle, _ptr(cat), _ptr(fl), self.n_item, n_cat, _ptr(t_off), _ptr(t_pc), _ptr(t_need), _ptr(t_any),
                                                 _ptr(t_forbid), P, _ptr(bits), W, _ptr(cnt), self._stream()))
        counts = cnt.cpu().numpy()
        bad = self.ctx.take_bad_ids(self._stream().value)
        if bad:
            raise IndexError("%d POI(s) with a category outside [0, %d): they pass no predicate that lists categories" % (bad, n_cat))
        return PoiFilter(self, bits, counts)

    def _filtered_args(self, k, filt, which, n, path):
        """(k, per-row predicate tensor or None, cand_hint, path code) of a filtered call, host arguments checked."""
        k = int(k)
        if not 1 <= k <= self.FILTER_K_MAX:
            raise ValueError("filtered recommendation supports 1 <= k <= %d (got %d)" % (self.FILTER_K_MAX, k))
        self._check_filter(filt)
        if path not in self._FILTER_PATH:
            raise ValueError("path must be one of %s (got %r)" % (", ".join(repr(p) for p in self._FILTER_PATH), path))
        pred, hint = self._which_arg(filt, which, n)
        return k, pred, hint, self._FILTER_PATH[path]

    def _check_filter(self, filt):
        if not isinstance(filt, PoiFilter) or filt.n_item != self.n_item or filt.bits.device != self.device:
            raise ValueError("filt must be a PoiFilter built for this model (model.poi_filter / PoiFilter.from_masks)")

    def _which_arg(self, filt, which, n):
        """which -> (the per-row predicate tensor, or None: predicate 0; the most POIs a named predicate passes)."""
        if which is None:
            return None, int(filt.counts[0])
        if isinstance(which, torch.Tensor):      # a device tensor is checked by the kernel
            pred, hint = which.to(self.device, torch.int32).contiguous().reshape(-1), int(filt.counts.max())
        else:
            w = np.atleast_1d(np.asarray(which)).astype(np.int64)
            if w.size and (w.min() < 0 or w.max() >= filt.n_pred):
                raise IndexError("which must index the filter's %d predicate(s) (found %d..%d)" % (filt.n_pred, int(w.min()), int(w.max())))
            pred, hint = torch.as_tensor(w.astype(np.int32)).to(self.device), int(filt.counts[w].max()) if w.size else 0
        if pred.numel() != n:
            raise ValueError("which must hold one predicate index per row (%d vs %d)" % (pred.numel(), n))
        return pred, hint

    def _filtered_out(self, idx, sc, cnt, return_scores, return_counts, sync):
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync,
                               "row(s) with a predicate index, an anchor or an exclusion id out of range: their lists are all -1")

    def _filtered_launch(self, users, items, anchor, c_r, ex, term, filt, pred, hint, k, path, return_scores, return_counts, sync):
        """One poi_score_topk_filtered call -> idx[, scores][, counts] (device tensors).  term: compute_sub_topk_near's."""
        n = users.shape[0]
        radius = c_r < float("inf")
        coords = cphi = order = None
        if radius or term is not None:
            coords, cphi, order = self._near_geo(radius)
        wd, sts, thr, n_dist, dd_m = term if term is not None else (None, None, None, 0, 0.0)
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        if n:
            self.ctx.check(self.lib.poi_score_topk_filtered(self.ctx.handle, _ptr(users), _ptr(items), n, self.n_item, self.kdim, _ptr(wd), _ptr(sts),
                                                            _ptr(coords), _ptr(cphi), _ptr(thr), _ptr(anchor), int(n_dist), float(dd_m), _ptr(filt.bits),
                                                            filt.ldw, filt.n_pred, _ptr(pred), hint, _ptr(order), c_r, _ptr(ex[0]), _ptr(ex[1]), k, path,
                                                            _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        return self._filtered_out(idx, sc, cnt, return_scores, return_counts, sync and n > 0)

    def _filtered_from_scores(self, score_rows, n, ex, filt, pred, k, return_scores, return_counts, sync):
        """Explicit score rows, a bounded number of rows at a time, + poi_topk_filtered_scores.  score_rows(o, c) -> (c, n_item)
        float32 scores of rows o .. o + c - 1."""
        N = self.n_item
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        for o, c in self._row_chunks(n):
            full = score_rows(o, c).contiguous()
            self.ctx.check(self.lib.poi_topk_filtered_scores(self.ctx.handle, _ptr(full), c, N, N, _ptr(filt.bits), filt.ldw, filt.n_pred, _at(pred, o, 1),
                                                             _at(ex[0], o, 1), _ptr(ex[1]), k, _at(idx, o, k), _at(sc, o, k), _at(cnt, o, 1), self._stream()))
        return self._filtered_out(idx, sc, cnt, return_scores, return_counts, sync and n > 0)

    def compute_sub_topk_filtered(self, start_end, k, filt, which=None, within_km=None, exclude=None, anchor=None, path="auto",
                                  return_scores=False, return_counts=False, sync=True):
        """FILTERED top-K (include/poi_hip.h, poi_score_topk_filtered): compute_sub_topk over the POIs that pass a predicate of `filt`
        (model.poi_filter / PoiFilter.from_masks) - "the best restaurants for this user".  which: the predicate index of every row
        (default: predicate 0).  within_km / exclude / anchor as compute_sub_topk_near (default anchor: the user's last train POI; the
        anchor is a candidate only if it passes the predicate too); the spatial model's distance term is taken at the anchor.  path:
        "auto" (by the radius and the predicates' pass counts), "walk" or "gather" - the result is the same bits on either.  Returns
        (n, k) int32 ids (k <= 32) by descending score, ties by ascending id, -1 where fewer POIs pass (scores -inf; NaN and -inf
        scores are never listed, -0.0 is +0.0); with return_counts the number of passing candidates of every row.  CA-RNN, PRME, GeoIE
        and POI2Vec go through their own score rows, a bounded number at a time, and poi_topk_filtered_scores; a radius is not
        defined for them.  Host arguments are checked before the launch; device tensors by the kernel: an offending row comes out all
        -1 and - with sync - raises IndexError."""
        fused = self._near_ok and self._rank_fused
        src = self._source(start_end, ("train", "last") if fused else ("train",), fused)
        return self._serve_filtered(src, k, filt, which, within_km, exclude, anchor, path, return_scores, return_counts, sync)

    def _serve_filtered(self, src, k, filt, which, within_km, exclude, anchor, path, return_scores, return_counts, sync):
        """The filtered top-K of a source's rows: poi_score_topk_filtered around the anchor, or - no radius and no anchor there - its
        score rows + poi_topk_filtered_scores."""
        if within_km is not None or anchor is not None:
            src.need_fused("filtered")
        k, pred, hint, pathc = self._filtered_args(k, filt, which, src.n, path)
        if src.fused:
            anc = self._near_anchor(anchor, src.n, src.anchor)
            ex = src.exclusion(exclude, anc)
            out = self._filtered_launch(src.users, src.items, anc.contiguous(), self._near_radius(within_km), ex, src.near_term(), filt, pred, hint, k,
                                        pathc, return_scores, return_counts, sync)
        else:
            out = self._filtered_from_scores(src.score_rows(), src.n, src.exclusion(exclude), filt, pred, k, return_scores, return_counts, sync)
        return src.finish(out, return_scores, return_counts)


    # ---- capped recommendation (poi_labels_build / poi_score_topk_capped / poi_topk_capped_scores): top-K with at most `per` POIs per label
    CAPPED_K_MAX = 32
    CAPPED_PER_MAX = 32

    def poi_labels(self, labels, n_label=None, filt=None):
        """labels: (n_item) ints, numpy or torch - >= 0 the POI's group (a category, a chain, a grid cell of data.grid_labels), < 0
        unlabelled -> a PoiLabels.  n_label: labels lie below it (default: the largest label + 1); 1 <= n_label <= n_item.  filt: the
        PoiFilter the capped calls will use, so that the gate knows how long each predicate's lists can get.  One launch and one
        synchronisation (the per-label counts come to the host): a set-up step, like poi_filter.  Labels that arrive as a DEVICE
        tensor without n_label cost a second one, for their maximum; host labels give it on the host.  A label >= n_label raises
        IndexError."""
        host = None if isinstance(labels, torch.Tensor) else np.ascontiguousarray(np.asarray(labels).astype(np.int64))
        lab = labels if host is None else torch.as_tensor(host)
        if tuple(lab.shape) != (self.n_item,):
            raise ValueError("labels must hold one id per POI (%s vs n_item = %d)" % (tuple(lab.shape), self.n_item))
        if n_label is None:
            n_label = max(int(lab.max().item() if host is None else host.max()) + 1, 1)
        n_label = int(n_label)
        if not 1 <= n_label <= self.n_item:
            raise ValueError("n_label must lie in [1, n_item = %d] (got %d)" % (self.n_item, n_label))
        if filt is not None:
            self._check_filter(filt)
        lab = lab.to(device=self.device, dtype=torch.int32).contiguous()
        rows = filt.n_pred if filt is not None else 1
        fill = torch.empty((rows, self.CAPPED_PER_MAX + 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n_label, dtype=torch.int32, device=self.device)
        self.ctx.check(self.lib.poi_labels_build(self.ctx.handle, _ptr(lab), self.n_item, n_label, _ptr(filt.bits) if filt is not None else None,
                                                 filt.ldw if filt is not None else 0, filt.n_pred if filt is not None else 0, _ptr(cnt), _ptr(fill),
                                                 self._stream()))
        counts = cnt.cpu().numpy()
        bad = self.ctx.take_bad_ids(self._stream().value)
        if bad:
            raise IndexError("%d POI(s) with a label outside [.., %d): they would be ranked as unlabelled" % (bad, n_label))
        return PoiLabels(self, lab, n_label, fill, counts, filt)

    def _capped_args(self, k, labels, per, filt, which, n):
        """(k, per, PoiLabels, per-row predicate tensor or None, fill tensor or None) of a capped call, host arguments checked."""
        k, per = int(k), int(per)
        if not 1 <= k <= self.CAPPED_K_MAX:
            raise ValueError("capped recommendation supports 1 <= k <= %d (got %d)" % (self.CAPPED_K_MAX, k))
        if not 1 <= per <= self.CAPPED_PER_MAX:
            raise ValueError("capped recommendation supports 1 <= per <= %d (got %d)" % (self.CAPPED_PER_MAX, per))
        if filt is not None:
            self._check_filter(filt)
        if not isinstance(labels, PoiLabels):
            labels = self.poi_labels(labels, filt=filt)
        if labels.n_item != self.n_item or labels.labels.device != self.device:
            raise ValueError("labels must be a PoiLabels built for this model (model.poi_labels / PoiLabels.from_categories)")
        if filt is None and which is not None:
            raise ValueError("which indexes the predicates of filt: it needs one")
        pred = self._which_arg(filt, which, n)[0] if filt is not None else None
        # the fill table gates by predicate row: it serves the filter it was built with (without one: the call without a filter)
        fill = labels.fill if labels.filt is filt else None
        return k, per, labels, pred, fill

    def _capped_buffers(self, n, k, return_scores, return_labels, return_counts):
        idx, sc, cnt = self._topk_buffers(n, k, return_scores, return_counts)
        return idx, sc, (torch.empty((n, k), dtype=torch.int32, device=self.device) if return_labels else None), cnt

    def _capped_out(self, idx, sc, lab, cnt, return_scores, return_labels, return_counts, sync):
        return self._serve_out(idx, ((sc, return_scores), (lab, return_labels), (cnt, return_counts)), sync,
                               "row(s) with a predicate index, an anchor or an exclusion id out of range: their lists are all -1")

    def _capped_launch(self, users, items, term, ex, labels, per, fill, filt, pred, k, return_scores, return_labels, return_counts, sync):
        """One poi_score_topk_capped call -> idx[, scores][, labels][, counts] (device tensors).  term: (wd, sts rows, last POI rows) or
        None, as _candidates_launch takes it."""
        n = users.shape[0]
        idx, sc, lab, cnt = self._capped_buffers(n, k, return_scores, return_labels, return_counts)
        if n:
            bits, ldw, n_pred = (_ptr(filt.bits), filt.ldw, filt.n_pred) if filt is not None else (None, 0, 0)
            self.ctx.check(self.lib.poi_score_topk_capped(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(labels.labels), per,
                                                          _ptr(fill), bits, ldw, n_pred, _ptr(pred), _ptr(ex[0]), _ptr(ex[1]), k, _ptr(idx), _ptr(sc),
                                                          _ptr(lab), _ptr(cnt), self._stream()))
        return self._capped_out(idx, sc, lab, cnt, return_scores, return_labels, return_counts, sync and n > 0)

    def _capped_from_scores(self, score_rows, n, ex, labels, per, fill, filt, pred, k, return_scores, return_labels, return_counts, sync):
        """Explicit score rows, a bounded number of rows at a time, + poi_topk_capped_scores.  score_rows(o, c) -> (c, n_item) float32
        scores of rows o .. o + c - 1."""
        N = self.n_item
        idx, sc, lab, cnt = self._capped_buffers(n, k, return_scores, return_labels, return_counts)
        bits, ldw, n_pred = (_ptr(filt.bits), filt.ldw, filt.n_pred) if filt is not None else (None, 0, 0)
        for o, c in self._row_chunks(n):
            full = score_rows(o, c).contiguous()
            self.ctx.check(self.lib.poi_topk_capped_scores(self.ctx.handle, _ptr(full), c, N, N, _ptr(labels.labels), per, _ptr(fill), bits, ldw, n_pred,
                                                           _at(pred, o, 1), _at(ex[0], o, 1), _ptr(ex[1]), k, _at(idx, o, k), _at(sc, o, k), _at(lab, o, k),
                                                           _at(cnt, o, 1), self._stream()))
        return self._capped_out(idx, sc, lab, cnt, return_scores, return_labels, return_counts, sync and n > 0)

    def compute_sub_topk_capped(self, start_end, k, labels, per=1, filt=None, which=None, exclude=None, return_scores=False, return_labels=False,
                                return_counts=False, sync=True):
        """CAPPED top-K (include/poi_hip.h, poi_score_topk_capped): compute_sub_topk with at most `per` POIs of one label - "the best 20
        places, but no more than 2 of a category"; with per = 1, the best POI of each of the k best labels.  labels: a PoiLabels
        (model.poi_labels / PoiLabels.from_categories; a plain array is turned into one, at the price of a synchronisation).
        Unlabelled POIs (label < 0) are never capped.  filt / which: restrict the candidates to a predicate per row as
        compute_sub_topk_filtered does; build the PoiLabels with the same filt, or the gate falls back to k (correct, slower where
        lists cannot fill).  exclude: None, "train" or CSR lists (off, ids) as compute_sub_candidates.  Returns (n, k) int32 ids
        (k <= 32, per <= 32) by descending score under the model's own score (the spatial model's distance term at the user's last
        POI), ties by ascending id, -1 where the cap or the candidates leave fewer; with return_scores the scores (-inf on the fill),
        with return_labels the entries' labels (-1 on the fill), with return_counts the candidates of every row, not reduced by the
        cap.  CA-RNN, PRME, POI2Vec and GeoIE under rule="geo" go through their own score rows, a bounded number at a time, and
        poi_topk_capped_scores.  Host arguments are checked before the launch (ValueError / IndexError); device tensors by the
        kernel: an offending row comes out all -1 and - with sync - raises IndexError."""
        return self._serve_capped(self._source(start_end), k, labels, per, filt, which, exclude, return_scores, return_labels, return_counts, sync)

    def _serve_capped(self, src, k, labels, per, filt, which, exclude, return_scores, return_labels, return_counts, sync):
        """The capped top-K of a source's rows: poi_score_topk_capped, or its score rows + poi_topk_capped_scores."""
        k, per, labels, pred, fill = self._capped_args(k, labels, per, filt, which, src.n)
        ex = src.exclusion(exclude)
        if src.fused:
            out = self._capped_launch(src.users, src.items, src.tile_term(), ex, labels, per, fill, filt, pred, k, return_scores, return_labels,
                                      return_counts, sync)
        else:
            out = self._capped_from_scores(src.score_rows(), src.n, ex, labels, per, fill, filt, pred, k, return_scores, return_labels,
                                           return_counts, sync)
        return src.finish(out, return_scores, return_counts)

    # ---- label recommendation (poi_score_labels / poi_score_topk_labels / poi_labels_scores): the next category / district by probability mass
    LABELS_K_MAX = 32
    _LABELS_BY = {"mass": 0, "max": 1}
    _LABELS_BAD = "row(s) with an anchor or an exclusion id out of range: their label lists are all -1"

    def _labels_args(self, k, labels, by):
        """(k, PoiLabels, the library's code of `by`) of a label call, host arguments checked; k None: the dense call."""
        if k is not None:
            k = int(k)
            if not 1 <= k <= self.LABELS_K_MAX:
                raise ValueError("label recommendation supports 1 <= k <= %d (got %d)" % (self.LABELS_K_MAX, k))
        if by not in self._LABELS_BY:
            raise ValueError("by must be 'mass' or 'max' (got %r)" % (by,))
        if not isinstance(labels, PoiLabels):
            labels = self.poi_labels(labels)
        if labels.n_item != self.n_item or labels.labels.device != self.device:
            raise ValueError("labels must be a PoiLabels built for this model (model.poi_labels / PoiLabels.from_categories)")
        if self.n_item >= 1 << 27:
            raise ValueError("label recommendation supports n_item < 2^27 (got %d)" % self.n_item)
        return k, labels, self._LABELS_BY[by]

    def _labels_buffers(self, n, k, return_best):
        lab = torch.empty((n, k), dtype=torch.int32, device=self.device)
        logp = torch.empty((n, k), dtype=torch.float64, device=self.device)
        bid = torch.empty((n, k), dtype=torch.int32, device=self.device) if return_best else None
        bsc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_best else None
        return lab, logp, bid, bsc

    def _labels_launch(self, users, items, term, ex, labels, by, k, return_best, sync):
        """One poi_score_topk_labels call -> labels, logp[, best ids, best scores] (device tensors).  term: (wd, sts rows, last POI rows)
        or None, as _candidates_launch takes it."""
        n = users.shape[0]
        lab, logp, bid, bsc = self._labels_buffers(n, k, return_best)
        if n:
            self.ctx.check(self.lib.poi_score_topk_labels(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(labels.labels),
                                                          labels.n_label, _ptr(ex[0]), _ptr(ex[1]), by, k, _ptr(lab), _ptr(logp), _ptr(bid), _ptr(bsc),
                                                          None, None, None, None, self._stream()))
        return self._serve_out(lab, ((logp, True), (bid, return_best), (bsc, return_best)), sync and n > 0, self._LABELS_BAD)

    def _labels_from_scores(self, score_rows, n, ex, labels, by, k, return_best, sync):
        """Explicit score rows, a bounded number of rows at a time, + poi_labels_scores.  score_rows(o, c) -> (c, n_item) float32 scores
        of rows o .. o + c - 1."""
        N = self.n_item
        lab, logp, bid, bsc = self._labels_buffers(n, k, return_best)
        for o, c in self._row_chunks(n):
            full = score_rows(o, c).contiguous()
            self.ctx.check(self.lib.poi_labels_scores(self.ctx.handle, _ptr(full), c, N, N, _ptr(labels.labels), labels.n_label, _at(ex[0], o, 1),
                                                      _ptr(ex[1]), by, k, None, None, None, None, _at(lab, o, k), _at(logp, o, k), _at(bid, o, k),
                                                      _at(bsc, o, k), None, None, None, None, self._stream()))
        return self._serve_out(lab, ((logp, True), (bid, return_best), (bsc, return_best)), sync and n > 0, self._LABELS_BAD)

    def recommend_labels(self, start_end, k, labels, by="mass", exclude=None, return_best=False, sync=True):
        """The next LABELS (include/poi_hip.h, poi_score_topk_labels): the k (<= 32) categories / districts of `labels` (a PoiLabels:
        model.poi_labels / PoiLabels.from_categories / data.grid_labels) the next check-in most likely falls in.  by="mass": by the
        softmax mass of the label's POIs under the model's own score (the spatial model's distance term at the user's last POI) - the
        probability of the label; by="max": by the label's single best POI, the order of compute_sub_topk_capped(per=1).  exclude:
        None, "train" or CSR lists (off, ids): excluded POIs leave the masses and the normaliser.  Returns (labels (n, k) int32 with -1
        where fewer labels have a candidate, log-probabilities (n, k) float64 with -inf on the fill) and, with return_best, the listed
        labels' best POI ids and scores.  The unlabelled POIs are never listed; their mass is part of the normaliser.  CA-RNN, PRME,
        POI2Vec and GeoIE under rule="geo" go through their own score rows, a bounded number at a time, and poi_labels_scores.  Host
        arguments are checked before the launch (ValueError / IndexError); device tensors by the kernel: an offending row comes out
        all -1 and - with sync - raises IndexError."""
        return self._serve_labels(self._source(start_end), k, labels, by, exclude, return_best, sync)

    def _serve_labels(self, src, k, labels, by, exclude, return_best, sync):
        """The next labels of a source's rows: poi_score_topk_labels, or its score rows + poi_labels_scores."""
        k, labels, byc = self._labels_args(k, labels, by)
        ex = src.exclusion(exclude)
        if src.fused:
            return self._labels_launch(src.users, src.items, src.tile_term(), ex, labels, byc, k, return_best, sync)
        return self._labels_from_scores(src.score_rows(), src.n, ex, labels, byc, k, return_best, sync)

    def label_distribution(self, start_end, labels, exclude=None):
        """The whole label distribution (poi_score_labels): ((n, n_label) float64 probabilities that the next check-in falls in each
        label, (n) float64 share of the unlabelled POIs) - the rows sum to 1 with the rest (a row without candidates is all zero).
        Arguments as recommend_labels; synchronises for the rejected-row count."""
        return self._serve_label_distribution(self._source(start_end), labels, exclude)

    def _serve_label_distribution(self, src, labels, exclude):
        """The dense label mass of a source's rows (poi_score_labels, or its score rows + poi_labels_scores) -> ((n, n_label) float64
        probabilities, (n) unlabelled rest)."""
        _, labels, _ = self._labels_args(None, labels, "mass")
        n, N, L = src.n, self.n_item, labels.n_label
        ex = src.exclusion(exclude)
        mass = torch.zeros((n, L + 1), dtype=torch.int64, device=self.device)      # (uint64 below 2^63: the same bits)
        if not src.fused:
            score_rows = src.score_rows()
            for o, c in self._row_chunks(n):
                full = score_rows(o, c).contiguous()
                self.ctx.check(self.lib.poi_labels_scores(self.ctx.handle, _ptr(full), c, N, N, _ptr(labels.labels), L, _at(ex[0], o, 1), _ptr(ex[1]), 0, 0,
                                                          _at(mass, o, L + 1), None, None, None, None, None, None, None, None, None, None, None,
                                                          self._stream()))
        elif n:
            self.ctx.check(self.lib.poi_score_labels(self.ctx.handle, *self._tile_operands(src.users, src.items, self.kdim, src.tile_term()),
                                                     _ptr(labels.labels), L, _ptr(ex[0]), _ptr(ex[1]), _ptr(mass), None, None, None, None, None,
                                                     self._stream()))
        if n and self.ctx.take_bad_ids(self._stream().value):
            raise IndexError("label_distribution: " + self._LABELS_BAD)
        m = mass.double()
        prob = m / m.sum(dim=1, keepdim=True).clamp(min=1.0)
        return prob[:, :L].contiguous(), prob[:, L].contiguous()


    # ---- group recommendation (poi_group_topk / poi_group_topk_scores): the top-K of an aggregate of the members' scores ---------------
    _GROUP_AGG = {"mean": 0, "min": 1}

    @staticmethod
    def _group_csr(groups, hi, what):
        """groups -> (off, ids, on_device): int64 host arrays.  A tuple (off, ids) is a CSR, anything else a list of id lists.  Host data
        is checked here (ValueError / IndexError before any launch).  Of a device CSR only the offsets' range is checked (they address
        memory; reading them is one sync): the order of its offsets and its ids are left to the kernel."""
        on_device = False
        if isinstance(groups, tuple) and len(groups) == 2:
            off, ids = groups
            on_device = isinstance(off, torch.Tensor) and isinstance(ids, torch.Tensor) and (off.is_cuda or ids.is_cuda)
            off = np.asarray(off.cpu().numpy() if isinstance(off, torch.Tensor) else off, np.int64).reshape(-1)
            ids = np.asarray(ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids, np.int64).reshape(-1)
            if len(off) < 1 or off.min() < 0 or off.max() > len(ids):
                raise ValueError("%s=(off, ids): the offsets must lie in [0, len(ids) = %d]" % (what, len(ids)))
            if not on_device and (off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0)):
                raise ValueError("%s=(off, ids): off must hold ascending offsets from 0 to len(ids) = %d" % (what, len(ids)))
        else:
            lists = [np.atleast_1d(np.asarray(g, np.int64)).reshape(-1) for g in groups]
            off = np.zeros(len(lists) + 1, np.int64)
            np.cumsum([len(g) for g in lists], out=off[1:])
            ids = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        if not on_device and ids.size and (ids.min() < 0 or ids.max() >= hi):
            raise IndexError("%s: ids must lie in [0, %d) (found %d..%d)" % (what, hi, int(ids.min()), int(ids.max())))
        return off, ids, on_device

    @staticmethod
    def _group_members(ids, hi):
        """(distinct valid ids ascending, member -> index into them; -1 for an id outside [0, hi): the kernel rejects that group)."""
        valid = (ids >= 0) & (ids < hi)
        uniq, inv = np.unique(ids[valid], return_inverse=True)
        mem = np.full(len(ids), -1, np.int32)
        mem[valid] = inv.astype(np.int32)
        return uniq, mem

    def _group_args(self, k, agg):
        k = int(k)
        if not 1 <= k <= 32:
            raise _lib.PoiError("group recommendation supports 1 <= k <= 32 (got %d)" % k)
        if agg not in self._GROUP_AGG:
            raise ValueError("agg must be 'mean' or 'min' (got %r)" % (agg,))
        return k, self._GROUP_AGG[agg]

    def _group_exclusion(self, exclude, off, ids, n_grp, kinds=("train",)):
        """exclude -> (ex_off (n_grp + 1), ex) int32 device tensors, or (None, None): ONE list per group."""
        if isinstance(exclude, str) and exclude == "train" and "train" in kinds:
            from .data import group_exclusion_csr
            host = self.__dict__.get("_near_train_host")
            if host is None:
                host = self._near_train_host = tuple(t.cpu().numpy() for t in self.train_exclusion())
            eo, ex = group_exclusion_csr(host[0], host[1], off, ids, self.n_item)      # (checks the lists on the host, device tensors included)
            i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
            return i32(eo), self._some_ids(i32(ex))
        return self._near_exclusion(exclude, n_grp, None, kinds=())

    def _group_out(self, idx, sc, cnt, return_scores, return_counts, sync):
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync,
                               "group(s) with a member out of range, descending offsets or a malformed exclusion list: their lists are all -1")

    def _group_launch(self, users, items, term, g_off, g_mem, n_grp, agg, ex, k, return_scores, return_counts, sync):
        """One poi_group_topk call -> idx[, scores][, counts] (device tensors).  term: (wd, sts rows, last POI rows) or None."""
        idx = torch.empty((n_grp, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n_grp, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n_grp, dtype=torch.int32, device=self.device) if return_counts else None
        self.ctx.check(self.lib.poi_group_topk(self.ctx.handle, *self._tile_operands(users, items, self.kdim, term), _ptr(g_off), _ptr(g_mem), n_grp,
                                               agg, _ptr(ex[0]), _ptr(ex[1]), k, _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        return self._group_out(idx, sc, cnt, return_scores, return_counts, sync)

    def _group_from_scores(self, off, ids, agg, ex, k, return_scores, return_counts, sync):
        """Explicit score rows (_rank_score_rows), whole groups at a time within the _rank_chunk budget of rows, + poi_group_topk_scores."""
        n_grp = len(off) - 1
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        idx = torch.empty((n_grp, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n_grp, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n_grp, dtype=torch.int32, device=self.device) if return_counts else None
        valid = (ids >= 0) & (ids < self.n_user)
        budget = self._rank_chunk(max(int(np.unique(ids[valid]).size), 1))
        rows_of = lambda g: ids[off[g]:off[g + 1]][valid[off[g]:off[g + 1]]] if off[g + 1] > off[g] else ids[:0]
        g = 0
        while g < n_grp:
            seen = set(rows_of(g).tolist())
            if len(seen) > budget:
                raise _lib.PoiError("group %d has %d distinct members: above the %d score rows one call may build" % (g, len(seen), budget))
            g2 = g + 1
            while g2 < n_grp:
                more = seen | set(rows_of(g2).tolist())
                if len(more) > budget:
                    break
                seen, g2 = more, g2 + 1
            a = np.array(sorted(seen), np.int64)
            full = self._own_score_rows(a)(0, len(a)).contiguous() if len(a) else None
            lo_, hi_ = int(off[g]), int(max(off[g2], off[g]))
            sub, ok = ids[lo_:hi_], valid[lo_:hi_]
            mem = np.full(hi_ - lo_, -1, np.int32)
            mem[ok] = np.searchsorted(a, sub[ok]).astype(np.int32)
            g_off, g_mem = i32(off[g:g2 + 1] - off[g]), self._some_ids(i32(mem))
            eo = ex[0][g:g2 + 1].contiguous() if ex[0] is not None else None
            self.ctx.check(self.lib.poi_group_topk_scores(self.ctx.handle, _ptr(full), len(a), self.n_item, _ptr(g_off), _ptr(g_mem), g2 - g, agg,
                                                          _ptr(eo), _ptr(ex[1]), k, _at(idx, g, k), _at(sc, g, k), _at(cnt, g, 1), self._stream()))
            g = g2
        return self._group_out(idx, sc, cnt, return_scores, return_counts, sync)

    def recommend_group(self, groups, k, agg="mean", exclude=None, return_scores=False, return_counts=False, sync=True):
        """Top-K for PARTIES of users (include/poi_hip.h, poi_group_topk): every POI is scored for every member with the model's own rule
        and the members' scores are aggregated - agg="mean" (the float32 sum in list order divided by the group size) or agg="min" (least
        misery: the score of the unhappiest member) - without the (members, n_item) score matrix.  groups: a list of lists of user ids,
        or a CSR pair (off, ids); a user listed twice counts twice.  exclude: None, "train" (the sorted union of the members' distinct
        train POIs leaves the ranking: data.group_exclusion_csr) or CSR lists (off, ids), ONE list per group, ids ascending and unique.
        Returns (n_grp, k) int32 ids by descending aggregate (k <= 32), ties by ascending id, -1 where a group has fewer than k
        candidates (scores -inf); with return_counts the candidate count of every group.  An empty group is all -1, count 0.
        Host arguments are checked before the launch; device tensors are checked by the kernel: an offending group comes out all -1
        and - with sync - raises IndexError (sync=False leaves the count to ctx.take_bad_ids()).  The models that score by
        users . items gather each distinct member's row once and take the fused kernel; CA-RNN, PRME, POI2Vec (the score of the
        user's next position) and GeoIE under rule="geo" go through their own score rows, whole groups at a time, and
        poi_group_topk_scores."""
        k, agg = self._group_args(k, agg)
        off, ids, on_device = self._group_csr(groups, self.n_user, "groups")
        n_grp = len(off) - 1
        ex = self._group_exclusion(exclude, off, ids, n_grp)
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        fused = self._rank_fused
        if n_grp == 0:
            return self._group_out(torch.empty((0, k), dtype=torch.int32, device=self.device), torch.empty((0, k), dtype=torch.float32, device=self.device),
                                   torch.empty(0, dtype=torch.int32, device=self.device), return_scores, return_counts, False)
        if not fused:
            return self._group_from_scores(off, ids, agg, ex, k, return_scores, return_counts, sync)
        uniq, mem = self._group_members(ids, self.n_user)
        if len(uniq):
            uid, users, lo = self._users_rows(uniq)
            term = self._rank_term(uid, lo)
        else:                                            # no valid member anywhere: nothing is gathered, every group is empty or rejected
            users, term = torch.zeros((0, self.kdim), dtype=torch.float32, device=self.device), None
        g_mem = self._some_ids(i32(mem))
        return self._group_launch(users.contiguous(), self._items(), term, i32(off), g_mem, n_grp, agg, ex, k, return_scores, return_counts, sync)


    # ---- audience recommendation (poi_score_audience / poi_audience_rows): given a POI, which users? -----------------------------------
    AUDIENCE_K_FUSED = 32       # the fused walk's list length; beyond it: score rows + poi_topk_select

    def train_visitors(self):
        """Every POI's DISTINCT train visitors as a sorted CSR (voff (n_item + 1) int32, user ids int32) on the device - built once and
        cached (data.visitors_csr): the exclude="train" lists of recommend_audience."""
        t = self.__dict__.get("_audience_train")
        if t is None:
            if getattr(self, "_off_host", None) is None or getattr(self, "p", None) is None:
                raise _lib.PoiError("%s keeps no (off, p) train table: pass the visitor lists as exclude=(off, ids)" % type(self).__name__)
            from .data import visitors_csr
            vo, us = visitors_csr(self._off_host, self.p.cpu().numpy(), self.n_item)
            self._audience_train_host = (vo, us)
            i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
            t = self._audience_train = (i32(vo), self._some_ids(i32(us)))
        return t

    def _audience_k(self, k, n, fused):
        k = int(k)
        if not (1 <= k <= min(self.CANDIDATES_K_MAX, n) or (fused and 1 <= k <= self.AUDIENCE_K_FUSED)):
            raise ValueError("audience recommendation supports 1 <= k <= min(%d, candidates = %d)%s (got %d)"
                             % (self.CANDIDATES_K_MAX, n, ", or k <= 32 whatever the candidate count" if fused else "", k))
        return k

    def _audience_queries(self, pois, host=False):
        """pois -> int32 device tensor (n_q).  Host ids are range-checked (IndexError before any launch); a device tensor is left to the
        kernel - unless `host`: the caller gathers with the ids on the host side of things and needs them checked."""
        if isinstance(pois, torch.Tensor) and pois.is_cuda and not host:
            return pois.to(self.device, torch.int32).reshape(-1).contiguous()
        a = np.atleast_1d(np.asarray(pois.cpu().numpy() if isinstance(pois, torch.Tensor) else pois)).astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= self.n_item):
            raise IndexError("pois must lie in [0, %d) (found %d..%d)" % (self.n_item, int(a.min()), int(a.max())))
        return torch.as_tensor(a.astype(np.int32)).to(self.device)

    @staticmethod
    def _audience_segment(users, hi, what="users"):
        """users -> None (every row) or the ascending unique int64 host id list of a segment (ValueError / IndexError)."""
        if users is None:
            return None
        a = np.atleast_1d(np.asarray(users.cpu().numpy() if isinstance(users, torch.Tensor) else users)).astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= hi):
            raise IndexError("%s must lie in [0, %d) (found %d..%d)" % (what, hi, int(a.min()), int(a.max())))
        if a.size > 1 and np.any(np.diff(a) <= 0):
            raise ValueError("%s must be strictly ascending (sorted, unique)" % what)
        return a

    def _audience_exclusion(self, exclude, q, seg, n_all, kinds=("train",)):
        """exclude -> (ex_off (n_q + 1), ex) int32 device tensors of ROW INDICES per query, or (None, None).  seg: the segment's ids
        (the lists are restricted to it and re-indexed), or None (row index = id)."""
        n_q = q.numel()
        empty = self._some_ids
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        if exclude is None:
            return None, None
        if isinstance(exclude, str):
            if exclude not in kinds:
                raise ValueError("exclude must be None, %s or a pair (off, ids) (got %r)" % (", ".join(repr(k) for k in kinds) or "-", exclude))
            vo, us = self.train_visitors()
            if seg is None:                                     # gather the queried POIs' lists on the device (a bad id lists nothing)
                ok = (q >= 0) & (q < self.n_item)
                qc = q.long().clamp(0, self.n_item - 1)
                beg, ln = vo[qc].long(), (vo[qc + 1] - vo[qc]).long() * ok.long()
                no = torch.zeros(n_q + 1, dtype=torch.int64, device=self.device)
                no[1:] = torch.cumsum(ln, 0)
                pos = torch.arange(int(no[-1].item()), device=self.device) - torch.repeat_interleave(no[:-1] - beg, ln)
                return no.int(), (us[pos].contiguous() if pos.numel() else empty())
            off, lst = self._audience_train_host
            qh = q.cpu().numpy().astype(np.int64)
            okh = (qh >= 0) & (qh < self.n_item)
            qh = np.clip(qh, 0, self.n_item - 1)
            ln = (off[qh + 1] - off[qh]) * okh
            pos = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln - off[qh], ln)
            off, lst = np.concatenate(([0], np.cumsum(ln))), lst[pos].astype(np.int64)
        else:
            off, lst = exclude
            if isinstance(off, torch.Tensor) and isinstance(lst, torch.Tensor) and seg is None:      # device lists are checked by the kernel
                if off.numel() != n_q + 1:
                    raise ValueError("exclude=(off, ids): off must hold n_q + 1 = %d offsets" % (n_q + 1))
                lst = lst.to(self.device, torch.int32).contiguous()
                return off.to(self.device, torch.int32).contiguous(), (lst if lst.numel() else empty())
            off = off.cpu().numpy() if isinstance(off, torch.Tensor) else off
            lst = lst.cpu().numpy() if isinstance(lst, torch.Tensor) else lst
            from .data import check_exclusion_csr
            off, lst = (np.asarray(v, np.int64) for v in check_exclusion_csr(off, lst, n_q, n_all))
            if seg is None:
                return i32(off), (i32(lst) if len(lst) else empty())
        # restricted to the segment and re-indexed: the rows keep the lists' ascending order
        at = np.searchsorted(seg, lst)
        keep = (at < len(seg)) & (seg[np.minimum(at, max(len(seg) - 1, 0))] == lst) if len(seg) else np.zeros(len(lst), bool)
        row = np.repeat(np.arange(n_q), np.diff(off))
        no = np.zeros(n_q + 1, np.int64)
        np.cumsum(np.bincount(row[keep], minlength=n_q), out=no[1:])
        return i32(no), (i32(at[keep]) if keep.any() else empty())

    def _audience_out(self, idx, sc, cnt, seg_dev, return_scores, return_counts, sync):
        if seg_dev is not None and idx.numel():                 # row indices -> ids; -1 stays -1
            idx = torch.where(idx >= 0, seg_dev[idx.clamp(min=0).long()], idx)
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync,
                               "query POI(s) outside [0, %d) or with a malformed exclusion list: their lists are all -1" % self.n_item)

    def _audience_select(self, buf, c, n, ld, k, ex, o, idx, sc, cnt):
        """poi_topk_select over the (c, ld) score rows of queries o .. o + c - 1: there the rows are the queries, the "items" the n candidates."""
        self.ctx.check(self.lib.poi_topk_select(self.ctx.handle, _ptr(buf), c, n, ld, k, _at(ex[0], o, 1), _ptr(ex[1]), _at(idx, o, k), _at(sc, o, k), _at(cnt, o, 1),
                                                self._stream()))

    def _audience_launch(self, users, items, kdim, term, q, ex, k, seg_dev, return_scores, return_counts, sync):
        """The fused paths on explicit candidate rows `users` (n, kdim): one poi_score_audience call for k <= 32, poi_audience_rows into a
        bounded buffer + poi_topk_select beyond.  term: (wd, sts rows, last POI rows) or None."""
        n, n_q = users.shape[0], q.numel()
        idx = torch.empty((n_q, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n_q, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n_q, dtype=torch.int32, device=self.device) if return_counts else None
        ops = self._tile_operands(users, items, kdim, term)
        if n_q and k <= self.AUDIENCE_K_FUSED:
            self.ctx.check(self.lib.poi_score_audience(self.ctx.handle, *ops, _ptr(q), n_q, _ptr(ex[0]), _ptr(ex[1]), k, _ptr(idx), _ptr(sc), _ptr(cnt),
                                                       self._stream()))
        elif n_q:
            ld = (n + 31) // 32 * 32
            per = max(1, min(n_q, self.SCORE_ROWS_BYTES // (4 * ld)))
            buf = torch.empty((per, ld), dtype=torch.float32, device=self.device)
            for o in range(0, n_q, per):                        # (no host synchronisation between the chunks)
                c = min(per, n_q - o)
                self.ctx.check(self.lib.poi_audience_rows(self.ctx.handle, *ops, ctypes.c_void_p(q.data_ptr() + 4 * o), c, _ptr(buf), ld, self._stream()))
                self._audience_select(buf, c, n, ld, k, ex, o, idx, sc, cnt)
            if cnt is not None:                                 # a rejected query's row is -inf: nothing is listed, and nothing counted
                cnt = torch.where((q >= 0) & (q < self.n_item), cnt, torch.zeros_like(cnt))
        return self._audience_out(idx, sc, cnt, seg_dev, return_scores, return_counts, sync and n_q > 0)

    def _audience_from_scores(self, a, q, ex, k, seg_dev, return_scores, return_counts, sync):
        """The models that rank by a rule of their own: their score rows (_own_score_rows) of the users `a`, _rank_chunk users at a time;
        the queried columns are gathered and transposed into the (queries, n) buffer, then poi_topk_select."""
        n, n_q = len(a), q.numel()
        idx = torch.empty((n_q, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n_q, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n_q, dtype=torch.int32, device=self.device) if return_counts else None
        ld = (n + 31) // 32 * 32
        per = max(1, min(max(n_q, 1), self.SCORE_ROWS_BYTES // (4 * ld)))
        score_rows = self._own_score_rows(a)
        buf = torch.empty((per, ld), dtype=torch.float32, device=self.device)
        for o in range(0, n_q, per):
            c = min(per, n_q - o)
            ql = q[o:o + c].long()
            for uo, uc in self._row_chunks(n):
                buf[:c, uo:uo + uc] = score_rows(uo, uc).index_select(1, ql).t()
            self._audience_select(buf, c, n, ld, k, ex, o, idx, sc, cnt)
        return self._audience_out(idx, sc, cnt, seg_dev, return_scores, return_counts, sync and n_q > 0)

    def recommend_audience(self, pois, k, users=None, exclude=None, return_scores=False, return_counts=False, sync=True):
        """AUDIENCE recommendation (include/poi_hip.h, poi_score_audience): given a POI, which users?  For every query POI the top-k
        users under the model's own score - the score compute_sub_target_rank ranks POIs with, read along the other axis - without the
        (n_user, n_item) score matrix.  users: None = every user, or an ascending unique id list = that segment only.  exclude: None,
        "train" (the POI's distinct train visitors leave the ranking: data.visitors_csr, restricted to the segment) or a CSR pair
        (off, ids) of user ids per query, ascending and unique.  Returns (n_q, k) int32 USER IDS on the device by descending score, ties by
        ascending id, -1 where a POI has fewer than k candidates (scores -inf); with return_counts the candidate count of every query.
        The same POI may be queried twice.  1 <= k <= 32 is one fused call; 32 < k <= min(4096, candidates) goes through
        poi_audience_rows, a bounded number of queries at a time, and poi_topk_select.  Host arguments are checked before the launch
        (ValueError / IndexError); device tensors are checked by the kernel: an offending query comes out all -1 and - with sync -
        raises IndexError (sync=False leaves the count to ctx.take_bad_ids()).  CA-RNN, PRME / PRPRM, POI2Vec and GeoIE go through
        their own score rows (the score of the user's next position), _rank_chunk users at a time, and poi_topk_select for any k."""
        fused = bool(self._rank_fused)
        seg = self._audience_segment(users, self.n_user)
        n = self.n_user if seg is None else len(seg)
        k = self._audience_k(k, n, fused)
        q = self._audience_queries(pois, host=not fused)
        ex = self._audience_exclusion(exclude, q, seg, self.n_user)
        seg_dev = None if seg is None else torch.as_tensor(seg.astype(np.int32)).to(self.device)
        a = np.arange(self.n_user) if seg is None else seg
        if not fused:
            return self._audience_from_scores(a, q, ex, k, seg_dev, return_scores, return_counts, sync)
        if n:
            ids, rows, lo = self._users_rows(a)
            term = self._rank_term(ids, lo)
        else:
            rows, term = torch.zeros((0, self.kdim), dtype=torch.float32, device=self.device), None
        return self._audience_launch(rows.contiguous(), self._items(), self.kdim, term, q, ex, k, seg_dev, return_scores, return_counts, sync)

    # ---- similar POIs and users (poi_similar_topk / poi_similar_rows / poi_similar_nearest): rows like this one ---------------------------
    SIMILAR_K_FUSED = 32        # the fused entry's list length; beyond it: similarity rows + poi_topk_select

    def _similar_args(self, k, n, geo_weight, scale_km):
        k, geo_weight, scale_km = int(k), float(geo_weight), float(scale_km)
        if not (1 <= k <= min(self.CANDIDATES_K_MAX, n - 1) or 1 <= k <= self.SIMILAR_K_FUSED):
            raise ValueError("similar rows support 1 <= k <= min(%d, rows - 1 = %d), or k <= 32 whatever the row count (got %d)"
                             % (self.CANDIDATES_K_MAX, n - 1, k))
        if not 0.0 <= geo_weight < 1.0:
            raise ValueError("geo_weight must lie in [0, 1) (got %r)" % (geo_weight,))
        if not scale_km > 0.0:
            raise ValueError("scale_km must be positive (got %r)" % (scale_km,))
        return k, geo_weight, scale_km

    def _similar_queries(self, ids, n, what):
        """ids -> int32 device tensor (n_q).  Host ids are range-checked (IndexError before any launch); a device tensor is left to the kernel."""
        if isinstance(ids, torch.Tensor) and ids.is_cuda:
            return ids.to(self.device, torch.int32).reshape(-1).contiguous()
        a = np.atleast_1d(np.asarray(ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids)).astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= n):
            raise IndexError("%s must lie in [0, %d) (found %d..%d)" % (what, n, int(a.min()), int(a.max())))
        return torch.as_tensor(a.astype(np.int32)).to(self.device)

    def _similar_launch(self, x, n, coords, cphi, q, ex, k, geo_weight, scale_km, what, return_scores, return_counts, sync):
        """The rows of x[:n] most similar to x[q]: one poi_similar_topk call for k <= 32; beyond, poi_similar_rows into a bounded buffer, a
        number of queries at a time, + poi_topk_select (no host synchronisation between the chunks)."""
        n_q, dim = q.numel(), x.shape[1]
        if dim % 4 or dim > 256:
            raise _lib.PoiError("the similarity supports rows of a multiple of 4 up to 256 columns (got %d)" % dim)
        idx = torch.empty((n_q, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n_q, k), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n_q, dtype=torch.int32, device=self.device) if return_counts else None
        head = [self.ctx.handle, _ptr(x), n, dim, _ptr(coords), _ptr(cphi), geo_weight, scale_km]
        if n_q and k <= self.SIMILAR_K_FUSED:
            self.ctx.check(self.lib.poi_similar_topk(*head, None, _ptr(q), n_q, _ptr(ex[0]), _ptr(ex[1]), k, _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        elif n_q:
            inv = torch.empty(n, dtype=torch.float64, device=self.device)
            self.ctx.check(self.lib.poi_row_inv_norms(self.ctx.handle, _ptr(x), n, dim, _ptr(inv), self._stream()))
            ld = (n + 31) // 32 * 32
            per = max(1, min(n_q, self.SCORE_ROWS_BYTES // (4 * ld)))
            buf = torch.empty((per, ld), dtype=torch.float32, device=self.device)
            for o in range(0, n_q, per):
                c = min(per, n_q - o)
                self.ctx.check(self.lib.poi_similar_rows(*head, _ptr(inv), ctypes.c_void_p(q.data_ptr() + 4 * o), c, _ptr(buf), ld, self._stream()))
                self._audience_select(buf, c, n, ld, k, ex, o, idx, sc, cnt)
            if cnt is not None:
                # the selection counted [0, n) minus the list: the query's own row leaves the count unless the list named it; a rejected
                # query's row is -inf: nothing is listed, and nothing counted
                named = torch.zeros(n_q + 1, dtype=torch.int32, device=self.device)
                if ex[0] is not None:
                    row = torch.bucketize(torch.arange(ex[1].numel(), device=self.device), ex[0][1:].long(), right=True)
                    hit = (row < n_q) & (ex[1] == q[row.clamp(max=n_q - 1)])
                    named.index_add_(0, row, hit.int())
                valid = (q >= 0) & (q < n)
                cnt = torch.where(valid, (cnt - 1 + named[:n_q].clamp(max=1)).clamp(min=0), torch.zeros_like(cnt))
        return self._serve_out(idx, ((sc, return_scores), (cnt, return_counts)), sync and n_q > 0,
                               "%s outside [0, %d) or with a malformed exclusion list: their lists are all -1" % (what, n))

    def similar_pois(self, pois, k, geo_weight=0.0, scale_km=1.0, exclude=None, return_scores=False, return_counts=False, sync=True):
        """PLACES LIKE THIS ONE (include/poi_hip.h, poi_similar_topk): for every query POI the k POIs most similar to it under
        sim = geo_weight * exp(-distance_km / scale_km) + (1 - geo_weight) * cosine(item rows) - the similarity of the MMR re-ranking
        (compute_sub_topk_diverse), taken over the whole catalogue, on the table the model scores with.  The query itself is no
        candidate; exclude: None or a CSR pair (off, ids) of POI ids per query, ascending and unique.  0 <= geo_weight < 1.  Returns
        (n_q, k) int32 POI ids on the device by descending similarity, ties by ascending id, -1 where a query has fewer than k candidates
        (scores -inf); with return_counts the candidate count of every query.  1 <= k <= 32 is one fused call; 32 < k <=
        min(4096, n_item - 1) goes through poi_similar_rows, a bounded number of queries at a time, and poi_topk_select.  It is a
        similarity of the model's POI rows, not a decomposition of any score.  Host arguments are checked before the launch
        (ValueError / IndexError); device tensors are checked by the kernel: an offending query comes out all -1 and - with sync -
        raises IndexError (sync=False leaves the count to ctx.take_bad_ids()).  Models without a single POI table refuse it."""
        n = self.n_item
        k, geo_weight, scale_km = self._similar_args(k, n, geo_weight, scale_km)
        items, _, coords, cphi = self._diverse_sim(geo_weight, self._diverse_items())
        q = self._similar_queries(pois, n, "pois")
        ex = self._audience_exclusion(exclude, q, None, n, kinds=())
        return self._similar_launch(items, n, coords, cphi, q, ex, k, geo_weight, scale_km, "query POI(s)", return_scores, return_counts, sync)

    def similar_users(self, users, k, exclude=None, return_scores=False, return_counts=False, sync=True):
        """USERS LIKE THIS ONE: similar_pois over the user rows the model scores with (_users_rows of every user), by the cosine alone.
        Offered by the models whose score is users . items; the others raise ValueError."""
        if not self._rank_fused:
            raise ValueError("%s ranks by a score rule of its own, not users . items: its user rows carry no cosine similarity" % type(self).__name__)
        n = self.n_user
        k, _, _ = self._similar_args(k, n, 0.0, 1.0)
        rows = self._users_rows(np.arange(n))[1].contiguous()
        q = self._similar_queries(users, n, "users")
        ex = self._audience_exclusion(exclude, q, None, n, kinds=())
        return self._similar_launch(rows, n, None, None, q, ex, k, 0.0, 1.0, "query user(s)", return_scores, return_counts, sync)

    def _similar_train(self):
        """Every user's train sequence as a CSR (off host int64, off int32, ids int32 on the device), padding ids (>= n_item) dropped; built once."""
        t = self.__dict__.get("_similar_train_csr")
        if t is None:
            if getattr(self, "_off_host", None) is None or getattr(self, "p", None) is None:
                raise _lib.PoiError("%s keeps no (off, p) train table: pass the histories as (off, ids)" % type(self).__name__)
            off, p = self._off_host.astype(np.int64), self.p.cpu().numpy().astype(np.int64)
            keep = (p >= 0) & (p < self.n_item)
            no = np.concatenate(([0], np.cumsum(keep)))[off]
            i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
            ids = p[keep]
            t = self._similar_train_csr = (no, ids, i32(no), self._some_ids(i32(ids)))
        return t

    def nearest_visited(self, start_end, lists, histories="train", geo_weight=0.0, scale_km=1.0, return_sims=False, sync=True):
        """BECAUSE YOU VISITED X (include/poi_hip.h, poi_similar_nearest): for every POI on a row's list - lists (n, k <= 32), -1 fill,
        typically the row's recommendations - the POI of the row's history it is most similar to, under compute_sub_topk_diverse's
        float64 similarity (0 <= geo_weight <= 1).  histories: "train" (the rows' train sequences) or a CSR pair (off, ids) of POI ids per
        row, in any order, duplicates allowed.  Returns (n, k) int32 history POI ids on the device, -1 where there is none (a -1 entry,
        an empty history)[, the (n, k) float64 similarities, -inf there]; ties go to the earlier history position.  This attributes a
        recommendation to the most similar visited POI - it does NOT decompose the model's score (Explainer.explain does).  Host arguments are checked before the
        launch; device tensors by the kernel (an offending row comes out all -1 and - with sync - raises IndexError)."""
        geo_weight, scale_km = float(geo_weight), float(scale_km)
        if not 0.0 <= geo_weight <= 1.0:
            raise ValueError("geo_weight must lie in [0, 1] (got %r)" % (geo_weight,))
        if not scale_km > 0.0:
            raise ValueError("scale_km must be positive (got %r)" % (scale_km,))
        items, kdim, coords, cphi = self._diverse_sim(geo_weight, self._diverse_items() if geo_weight < 1.0 else None)
        ids, lo = self._ids(start_end)
        n = ids.numel()
        if isinstance(lists, torch.Tensor) and lists.is_cuda:
            lt = lists.to(self.device, torch.int32)
        else:
            a = np.asarray(lists.cpu().numpy() if isinstance(lists, torch.Tensor) else lists).astype(np.int64)
            if a.size and (a.min() < -1 or a.max() >= self.n_item):
                raise IndexError("listed POIs must lie in [-1, %d) (found %d..%d)" % (self.n_item, int(a.min()), int(a.max())))
            lt = torch.as_tensor(a.astype(np.int32)).to(self.device)
        if lt.dim() != 2 or lt.shape[0] != n or not 1 <= lt.shape[1] <= 32:
            raise ValueError("lists must be (%d rows, 1 <= k <= 32) (got %s)" % (n, tuple(lt.shape)))
        lt, k = lt.contiguous(), lt.shape[1]
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        if isinstance(histories, str):
            if histories != "train":
                raise ValueError("histories must be 'train' or a pair (off, ids) (got %r)" % (histories,))
            off_h, ids_h, off_d, ids_d = self._similar_train()
            if lo is not None:                                  # a contiguous user range: its offsets index the cached ids as they are
                h_off, h_ids = off_d[lo:lo + n + 1], ids_d
            else:
                a = ids.cpu().numpy().astype(np.int64)
                ln = off_h[a + 1] - off_h[a]
                pos = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln - off_h[a], ln)
                h_off, h_ids = i32(np.concatenate(([0], np.cumsum(ln)))), self._some_ids(i32(ids_h[pos]))
        else:
            off, hid = histories
            if isinstance(off, torch.Tensor) and off.is_cuda and isinstance(hid, torch.Tensor) and hid.is_cuda:
                h_off, h_ids = off.to(self.device, torch.int32).contiguous(), hid.to(self.device, torch.int32).contiguous()
            else:
                off = np.asarray(off.cpu().numpy() if isinstance(off, torch.Tensor) else off).astype(np.int64).reshape(-1)
                hid = np.asarray(hid.cpu().numpy() if isinstance(hid, torch.Tensor) else hid).astype(np.int64).reshape(-1)
                if len(off) == 0 or off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] > len(hid):
                    raise ValueError("histories=(off, ids): off must ascend from >= 0 to at most len(ids)")
                if hid.size and (hid.min() < 0 or hid.max() >= self.n_item):
                    raise IndexError("history POIs must lie in [0, %d) (found %d..%d)" % (self.n_item, int(hid.min()), int(hid.max())))
                h_off, h_ids = i32(off), i32(hid)
            if h_off.numel() != n + 1:
                raise ValueError("histories=(off, ids): off must hold n + 1 = %d offsets" % (n + 1))
            if not h_ids.numel():
                h_ids = self._some_ids()
        pos = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sim = torch.empty((n, k), dtype=torch.float64, device=self.device) if return_sims else None
        if n:
            self.ctx.check(self.lib.poi_similar_nearest(self.ctx.handle, _ptr(items), self.n_item, kdim, _ptr(coords), _ptr(cphi), geo_weight, scale_km,
                                                        _ptr(lt), n, k, _ptr(h_off), _ptr(h_ids), _ptr(pos), _ptr(sim), self._stream()))
        at = (h_off[:-1].long()[:, None] + pos.clamp(min=0).long()).clamp(max=h_ids.numel() - 1)
        out = torch.where(pos >= 0, h_ids[at], torch.full_like(pos, -1))
        return self._serve_out(out, ((sim, return_sims),), sync and n > 0,
                               "row(s) with a listed or history POI outside [0, %d): their entries are all -1" % self.n_item)

    # ---- diversified recommendation (poi_diverse_topk / poi_diverse_rerank): a pool of the best candidates, re-ranked by MMR --------------
    def _diverse_items(self):
        """The POI rows the embedding similarity is taken between: the table the model scores with.  None: the model has no single POI
        table that means anything (geo_weight < 1 is then refused)."""
        return self._items()

    @staticmethod
    def _diverse_args(k, pool, trade, geo_weight, scale_km):
        k, pool, trade, geo_weight, scale_km = int(k), int(pool), float(trade), float(geo_weight), float(scale_km)
        if not 1 <= k <= 32:
            raise ValueError("diversified recommendation supports 1 <= k <= 32 (got %d)" % k)
        if not k <= pool <= 64:
            raise ValueError("pool must lie in [k, 64] (got pool %d, k %d)" % (pool, k))
        if not 0.0 <= trade <= 1.0:
            raise ValueError("trade must lie in [0, 1] (got %r)" % (trade,))
        if not 0.0 <= geo_weight <= 1.0:
            raise ValueError("geo_weight must lie in [0, 1] (got %r)" % (geo_weight,))
        if not scale_km > 0.0:
            raise ValueError("scale_km must be positive (got %r)" % (scale_km,))
        return k, pool, trade, geo_weight, scale_km

    def _diverse_sim(self, geo_weight, items):
        """(items, kdim, coords, cphi) of the similarity's two parts; a part with zero weight is not handed over."""
        coords = cphi = None
        if geo_weight > 0.0:
            coords, cphi, _ = self._near_geo(False)
        if geo_weight < 1.0:
            if items is None:
                raise ValueError("%s has no single POI table for an embedding similarity: use geo_weight=1" % type(self).__name__)
            items = items.contiguous()
            if items.shape[1] % 4 or items.shape[1] > 256:
                raise _lib.PoiError("the embedding similarity supports item rows of a multiple of 4 up to 256 columns (got %d)" % items.shape[1])
            return items, items.shape[1], coords, cphi
        return None, 0, coords, cphi

    def _diverse_out(self, idx, sc, obj, pool, cnt, return_scores, return_objective, return_pool, return_counts, sync):
        return self._serve_out(idx, ((sc, return_scores), (obj, return_objective), (pool, return_pool), (cnt, return_counts)), sync,
                               "row(s) with a malformed exclusion list or a pool id outside [0, %d): their lists are all -1" % self.n_item)

    def _diverse_buffers(self, n, k, pool, return_scores, return_objective, return_pool, return_counts):
        dev = self.device
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        sc = torch.empty((n, k), dtype=torch.float32, device=dev) if return_scores else None
        obj = torch.empty((n, k), dtype=torch.float64, device=dev) if return_objective else None
        pl = (torch.empty((n, pool), dtype=torch.int32, device=dev), torch.empty((n, pool), dtype=torch.float32, device=dev)) if return_pool else (None, None)
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if return_counts else None
        return idx, sc, obj, pl, cnt

    def _diverse_launch(self, users, items, kdim, term, ex, k, pool, trade, geo_weight, scale_km, return_scores, return_objective, return_pool,
                        return_counts, sync):
        """One poi_diverse_topk call.  term: (wd, sts rows, last POI rows) or None."""
        n = users.shape[0]
        idx, sc, obj, pl, cnt = self._diverse_buffers(n, k, pool, return_scores, return_objective, return_pool, return_counts)
        ops = self._tile_operands(users, items, kdim, term)
        if geo_weight > 0.0:                             # the re-ranking's geographic similarity needs coords / cphi without the term, too
            ops[7:9] = [_ptr(v) for v in self._near_geo(False)[:2]]
        self.ctx.check(self.lib.poi_diverse_topk(self.ctx.handle, *ops, _ptr(ex[0]), _ptr(ex[1]), pool, k, trade, geo_weight, scale_km, _ptr(idx),
                                                 _ptr(sc), None, _ptr(obj), _ptr(pl[0]), _ptr(pl[1]), _ptr(cnt), self._stream()))
        return self._diverse_out(idx, sc, obj, pl, cnt, return_scores, return_objective, return_pool, return_counts, sync)

    def _diverse_host_exclusion(self, ex, n):
        """The explicit-score path masks score rows with the lists: device lists are read back and checked like host lists."""
        if ex[0] is None:
            return ex
        from .data import check_exclusion_csr
        eo, ei = ex[0].cpu().numpy().astype(np.int64), ex[1].cpu().numpy()
        if len(eo) and 0 <= eo[0] <= eo[-1] <= len(ei):      # the rows' window of a longer id list (exclude="train" over a user range)
            eo, ei = eo - eo[0], ei[int(eo[0]):int(eo[-1])]
        eo, ei = check_exclusion_csr(eo, ei, n, self.n_item)
        return torch.as_tensor(eo).to(self.device), torch.as_tensor(ei).to(self.device)

    def _diverse_from_scores(self, score_rows, n, ex, sim, k, pool, trade, geo_weight, scale_km, return_scores, return_objective, return_pool,
                             return_counts, sync):
        """Explicit score rows, a bounded number of rows at a time: the exclusions masked to -inf, the pool from poi_topk, then
        poi_diverse_rerank.  score_rows(o, c) -> (c, n_item) float32 scores of rows o .. o + c - 1."""
        items, kdim, coords, cphi = sim
        N = self.n_item
        idx, sc, obj, pl, cnt = self._diverse_buffers(n, k, pool, return_scores, return_objective, True, return_counts)
        ex = self._diverse_host_exclusion(ex, n)
        kk = min(pool, N)
        ninf = float("-inf")
        for o, c in self._row_chunks(n):
            full = score_rows(o, c)
            full = torch.where(torch.isfinite(full), full, torch.full_like(full, ninf))      # NaN and +-inf are never pooled
            if ex[0] is not None:
                eo = ex[0][o:o + c + 1].long()
                ln = eo[1:] - eo[:-1]
                full[torch.repeat_interleave(torch.arange(c, device=self.device), ln), ex[1][int(eo[0]):int(eo[-1])].long()] = ninf
                if cnt is not None:
                    cnt[o:o + c] = (N - ln).int()
            elif cnt is not None:
                cnt[o:o + c] = N
            ti = torch.full((c, kk), -1, dtype=torch.int32, device=self.device)
            ts = torch.full((c, kk), ninf, dtype=torch.float32, device=self.device)
            self.ctx.check(self.lib.poi_topk(self.ctx.handle, _ptr(full.contiguous()), c, N, kk, _ptr(ti), _ptr(ts), self._stream()))
            dead = ~torch.isfinite(ts)
            ti[dead] = -1; ts[dead] = ninf
            pl[0][o:o + c] = -1; pl[1][o:o + c] = ninf
            pl[0][o:o + c, :kk] = ti; pl[1][o:o + c, :kk] = ts
            self.ctx.check(self.lib.poi_diverse_rerank(self.ctx.handle, _at(pl[0], o, pool), _at(pl[1], o, pool), c, pool, _ptr(items), N, kdim, _ptr(coords),
                                                       _ptr(cphi), k, trade, geo_weight, scale_km, _at(idx, o, k), _at(sc, o, k), None, _at(obj, o, k),
                                                       self._stream()))
        return self._diverse_out(idx, sc, obj, pl, cnt, return_scores, return_objective, return_pool, return_counts, sync)

    def compute_sub_topk_diverse(self, start_end, k, pool=64, trade=0.7, geo_weight=1.0, scale_km=1.0, exclude=None, return_scores=False,
                                 return_objective=False, return_pool=False, return_counts=False, sync=True):
        """DIVERSIFIED top-K (include/poi_hip.h, poi_diverse_topk): the `pool` best candidates of every row under the model's own score
        (k <= pool <= 64; exclude as compute_sub_topk_near: None, "train", "last" or CSR lists (off, ids)), re-ranked greedily for
        relevance against redundancy (maximal marginal relevance): the first pick is the best candidate, every further pick maximises
        trade * rel - (1 - trade) * (the largest similarity to a POI already picked), rel the pool's scores scaled to [0, 1].  The
        similarity is geo_weight * exp(-distance / scale_km) + (1 - geo_weight) * (cosine of the two item rows); a part with zero weight
        is not evaluated (geo_weight > 0 needs POI coordinates: set_coords).  trade = 1 is the plain top-K.  Returns (n, k) int32 ids
        (k <= 32), -1 where fewer candidates exist; with return_scores the picks' ORIGINAL scores, with return_objective the float64
        objective at selection, with return_pool the pair (pool ids, pool scores), with return_counts the candidate count of every row.
        No (n, n_item) matrix is built for the models that score by users . items; CA-RNN, PRME, POI2Vec and GeoIE under rule="geo" go
        through their own score rows, a bounded number at a time, poi_topk and poi_diverse_rerank.  Host arguments are checked before
        the launch (ValueError / IndexError)."""
        return self._serve_diverse(self._source(start_end, ("train", "last")), k, pool, trade, geo_weight, scale_km, exclude, return_scores,
                                   return_objective, return_pool, return_counts, sync)

    def _serve_diverse(self, src, k, pool, trade, geo_weight, scale_km, exclude, return_scores, return_objective, return_pool, return_counts, sync):
        """The diversified top-K of a source's rows: poi_diverse_topk, or its score rows + poi_topk + poi_diverse_rerank."""
        k, pool, trade, geo_weight, scale_km = self._diverse_args(k, pool, trade, geo_weight, scale_km)
        sim = self._diverse_sim(geo_weight, self._diverse_items() if geo_weight < 1.0 else None)
        flags = (return_scores, return_objective, return_pool, return_counts)
        ex = src.exclusion(exclude)
        if not src.fused:
            out = self._diverse_from_scores(src.score_rows(), src.n, ex, sim, k, pool, trade, geo_weight, scale_km, *flags, sync)
        elif src.n == 0:
            out = self._diverse_out(*self._diverse_buffers(0, k, pool, True, True, True, True), *flags, False)
        else:
            out = self._diverse_launch(src.users, src.items, src.kdim, src.tile_term(), ex, k, pool, trade, geo_weight, scale_km, *flags, sync)
        return src.finish(out, return_scores, return_counts)


# =================================================================================================
# ---- leave-one-out attribution (poi_explain_loo): the groups a history is cut into and the kernel's column tables ------------------------
def explain_groups(off, p, by):
    """The groups of GruBasic.explain over the CSR histories (off (n + 1) int64 from 0, p (total) ids; tensors of one device, torch ops
    only).  by="checkin": one group per position; by="poi": one per distinct POI of a row, numbered by first occurrence.  Returns
    (grp (total) int32 - the group of every position within its row, g_off (n + 1) int64 - row r owns the delta rows g_off[r] ..
    g_off[r + 1], keys (G) int32 - the POI every group removes, first (G) int64 - the group's first position within its row,
    row (G) int64)."""
    if by not in ("checkin", "poi"):
        raise ValueError("by must be 'checkin' or 'poi' (got %r)" % (by,))
    dev, n, total = p.device, off.numel() - 1, int(p.numel())
    off = off.to(dev, torch.int64)
    pos = torch.arange(total, device=dev)
    row = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1])
    local = pos - off[:-1][row]
    if by == "checkin":
        return local.int(), off.clone(), p.int(), local, row
    uniq, inv = torch.unique(row * (1 << 32) + (p.long() & 0xFFFFFFFF), return_inverse=True)      # (row, POI) pairs
    first = torch.full((uniq.numel(),), total, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, pos, "amin")
    order = torch.argsort(first)                                # first positions are distinct: row-major, first occurrence within a row
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=dev)
    at = first[order]
    g_row = row[at]
    g_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    g_off[1:] = torch.cumsum(torch.bincount(g_row, minlength=n), 0)
    return (rank[inv] - g_off[:-1][row]).int(), g_off, p[at].int(), local[at], g_row


def explain_columns(lens, g_off, first, row, start_mode=1):
    """The column tables of poi_explain_loo (include/poi_hip.h) for n rows of lengths `lens` and their groups (explain_groups; `row`
    counts from the first of these rows): int32 quadruples (row, key, start, 0).  base (n, 4): key -1, longest history first.
    variants (G, 4): key = the group within its row, start = 16 floor(first / 16) (start_mode 0: 0), longest remaining walk
    lens[row] - start first; equal lengths keep their order."""
    dev, n = lens.device, lens.numel()
    lens = lens.long()
    z = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
    b_order = torch.sort(-lens, stable=True)[1]
    base = torch.stack((b_order, z(n) - 1, z(n), z(n)), 1).int().contiguous()
    G = first.numel()
    key = torch.arange(G, device=dev) - g_off[:-1].long()[row]
    start = (first // 16) * 16 if start_mode else z(G)
    v_order = torch.sort(-(lens[row] - start), stable=True)[1]
    var = torch.stack((row, key, start, z(G)), 1)[v_order].int().contiguous()
    return base, var


class GruBasic(_Base):
    """public/GRU.py:32-205."""

    spatial = False

    _pad_ok = True          # dims other than 64 / 128 / 256 may be zero-padded to the next tile-engine dim (not CA-RNN: sigmoid(0) != 0)

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, device="cuda:0", init=None, seed=None, table_dtype="f32",
                 pad_dim=True):
        """pad_dim (default on): a model whose dim is not 64 / 128 / 256 (the reference's own configs use 20 and 32) is STORED with its
        hidden / embedding width zero-padded to the next of those, so that it trains on the MFMA tile engine instead of the
        per-sequence engine (dim 20: 1.5 M -> ~9 M sequences/s).  Exact: a padded hidden unit has zero weights and bias, so its gates
        are sigmoid(0), its candidate tanh(0) = 0 and its state stays 0; every gradient that touches a padded row or column is a
        product with one of those zeros, and the L2 decay of a zero is zero - the padding stays exactly zero and the other entries
        see only additional + 0.0 terms.  get_value / set_value / load_params / predict / checkpoints use the logical shapes.
        table_dtype="f16": the POI table `lt` and its evaluation snapshot are STORED as IEEE half (config X of BASELINE.json:
        "fp16 embeddings"); all arithmetic stays float32 - rows are converted when gathered and rounded to nearest-even when
        written back.  Tile engine only (dim 64 / 128 / 256).  NOTE: an update smaller than half an fp16 ulp of the element
        (2.4e-4 at 0.5) is lost to the rounding; with alpha 0.01 that is most single-sequence updates - use launches with a
        batch cap, whose summed updates are larger."""
        if n_in != n_hidden:
            raise ValueError("the reference drivers always pass n_in == n_hidden (prog_bpr_gru_spatial.py:138-139)")
        if table_dtype not in ("f32", "f16"):
            raise ValueError("table_dtype must be 'f32' or 'f16'")
        self.table_dtype = table_dtype
        self._setup(device, alpha_lambda)
        self.n_user, self.n_item, self.dim = int(n_user), int(n_item), int(n_in)
        D = self.dim
        self.kdim = D           # the dim the kernels see
        if pad_dim and self._pad_ok and D not in (64, 128, 256) and D < 256:
            self.kdim = 64 if D < 64 else 128 if D < 128 else 256
        self._load_tables(train, test)
        rng = np.random.default_rng(seed) if seed is not None else np.random
        u = lambda *s: rng.uniform(-0.5, 0.5, s)
        init = init or {}
        g = lambda k, v: (init[k] if isinstance(init[k], torch.Tensor) else np.asarray(init[k], np.float64)) if k in init else v()
        tdt = torch.float16 if table_dtype == "f16" else torch.float32
        sh = self._shared
        big = (n_item + 1) * D > (1 << 28) and self.kdim == D
        if big:
            # tables of hundreds of millions of elements (config X: 10 M x 256) are drawn ON the device: the host draw is 20 GB of float64
            gen = torch.Generator(device=self.device).manual_seed(0 if seed is None else int(seed))
            u_tab = lambda rows: (torch.rand((rows, D), generator=gen, device=self.device, dtype=torch.float32) - 0.5).to(tdt)
        else:
            u_tab = lambda rows: u(rows, D)
        self.lt = sh(g("lt", lambda: u_tab(n_item + 1)), "cols", tdt)                      # GRU.py:60
        self.ui = sh(g("ui", lambda: u(3, D, self._xw())), "ui")                           # :61 / GRU_Spatial.py:51
        self.wh = sh(g("wh", lambda: u(3, D, D)), "sq")                                    # :62
        self.bi = sh(g("bi", lambda: np.zeros((3, D))), "cols")                            # :64
        self.h0 = Shared(torch.zeros(self.kdim, dtype=torch.float32, device=self.device), unpad=(lambda a: a[:D]) if self.kdim != D else None)   # :63 never trained
        self.trained_items = sh(u_tab(n_item + 1), "cols", tdt)                            # :71
        self.trained_users = sh(u(n_user, D), "cols")                                      # :72
        if table_dtype == "f16":
            self.ctx.register_f16(self.lt.t); self.ctx.register_f16(self.trained_items.t)

    def __del__(self):
        try:
            if getattr(self, "table_dtype", "f32") == "f16":
                self.ctx.unregister_f16(self.lt.t); self.ctx.unregister_f16(self.trained_items.t)
        except Exception:
            pass

    def _xw(self):
        return self.dim

    def _shared(self, value, kind, dtype=torch.float32):
        """Device tensor of a parameter in the STORED layout (width kdim) with logical get / set.  kind: "cols" - last axis D -> kdim;
        "sq" - (3, D, D) -> (3, kdim, kdim); "ui" - (3, D, xw) with xw = D or 2 D column blocks, each block padded on its own."""
        D, K = self.dim, self.kdim
        if K == D:
            return Shared(self._dev(value, dtype))
        if kind == "cols":
            pad = lambda a: np.concatenate((a, np.zeros(a.shape[:-1] + (K - D,))), axis=-1)
            unpad = lambda a: a[..., :D]
        elif kind == "sq":
            def pad(a):
                o = np.zeros((3, K, K)); o[:, :D, :D] = a; return o
            unpad = lambda a: a[:, :D, :D]
        else:
            nb = self._xw() // D
            def pad(a):
                o = np.zeros((3, K, nb * K))
                for b in range(nb):
                    o[:, :D, b * K:b * K + D] = a[:, :, b * D:(b + 1) * D]
                return o
            unpad = lambda a: np.concatenate([a[:, :D, b * K:b * K + D] for b in range(nb)], axis=2)
        return Shared(self._dev(pad(np.asarray(value, np.float64)), dtype), pad=pad, unpad=unpad)

    def _pad_cols(self, t):
        """(n, D) or (n, kdim) device tensor -> (n, kdim)."""
        if t.shape[-1] == self.kdim:
            return t
        o = torch.zeros(t.shape[:-1] + (self.kdim,), dtype=t.dtype, device=t.device)
        o[..., :self.dim] = t
        return o

    def update_trained_users(self, all_hus):
        """public/GRU.py:89-91 ((n_user, D); the padded rows predict_device returns are taken as they are)."""
        t = all_hus if isinstance(all_hus, torch.Tensor) else self._dev(np.asarray(all_hus, np.float64))
        t = t.to(self.device, torch.float32).reshape(self.n_user, -1)
        self.trained_users.t.copy_(self._pad_cols(t))

    # ---- ctypes views ---------------------------------------------------------------------------
    def _params(self, snapshot=False):
        P = _lib.GruParams()
        P.lt = (self.trained_items if snapshot else self.lt).t.data_ptr()
        P.ui, P.wh, P.bi = self.ui.t.data_ptr(), self.wh.t.data_ptr(), self.bi.t.data_ptr()
        P.di = P.vs = P.bs = P.wd = P.lw = None
        P.n_item, P.n_dist, P.dim = self.n_item, 0, self.kdim
        return P

    def _tables(self):
        T = _lib.SeqTables()
        T.off, T.p, T.q = self.off.data_ptr(), self.p.data_ptr(), self.q.data_ptr()
        T.dp = T.dq = None
        T.n_user, T.len_max, T.max_len = self.n_user, self.len_max, self.max_len
        return T

    def session(self, n_slot=None):
        """Online state for this model (Session): per-slot h / last POI advanced one check-in at a time, top-K from it."""
        return Session(self, n_slot)

    def predict(self, idxs):
        """public/GRU.py:204-205 -> hts ndarray (n, D)."""
        return np.ascontiguousarray(self.predict_device(idxs)[:, :self.dim].cpu().numpy())

    def predict_device(self, idxs):
        """(n, kdim) device rows (kdim == dim unless the model is stored padded: the padding columns are zero)."""
        ids, out_row = self._by_length(idxs)
        n = ids.numel()
        hts = torch.empty((n, self.kdim), dtype=torch.float32, device=self.device)
        P, T = self._params(snapshot=True), self._tables()
        self.ctx.check(self.lib.poi_gru_predict(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), _ptr(out_row), n, _ptr(hts), None,
                                                self._stream()))
        return hts


class OboGru(GruBasic):
    """public/GRU.py:301-389 - plain GRU + BPR, one SGD step per user sequence."""

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, **kw):
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, **kw)
        self.params = [self.ui, self.wh, self.bi]
        self.l2 = _L2(self, ["lt", "ui", "wh", "bi"])                                      # :304-308

    def train(self, idx):
        """seq_train(uidx) -> float (public/GRU.py:387-389)."""
        return float(self.train_batch(np.atleast_1d(idx))[0])

    def train_batch(self, idxs, sync=True):
        """Throughput mode: n sequences per launch, batch semantics of include/poi_hip.h."""
        ids, _ = self._ids(idxs)
        n = ids.numel()
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        P, T = self._params(), self._tables()
        self.ctx.check(self.lib.poi_gru_step(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), n,
                                             self.alpha_lambda[0], self.alpha_lambda[1], _ptr(out), self._stream()))
        return out.cpu().numpy() if sync else out


class Gru(OboGru):
    """public/GRU.py:395-498 - the mini-batch GRU: `train(idxs)` takes a LIST of users and makes ONE SGD step on the cost
    -sum(loss) / batch + 0.5 lambda (every gathered row, ui, wh, bi) (:452-459).  Same kernels as OboGru with the launch as the
    mini-batch (poi_ctx_set_batch_cap(0), include/poi_hip.h): loss gradients averaged over the launch, L2 terms summed; predict /
    scoring / AUC are GruBasic's.  Returns -upq, the batch's summed loss (:473), like the reference."""

    def train(self, idxs):
        return float(np.sum(self.train_batch(idxs)))

    def train_batch(self, idxs, sync=True):
        prev = getattr(self.ctx, "batch_cap", 1.0)
        self.ctx.set_batch_cap(0.0)
        try:
            return super().train_batch(idxs, sync=sync)
        finally:
            self.ctx.set_batch_cap(prev)

    def normalize(self):
        """public/GRU.py:476-481: lt rows scaled to unit L2 norm (never called by the reference's drivers)."""
        t = self.lt.t.float()
        self.lt.t.copy_((t / t.pow(2).sum(dim=1, keepdim=True).sqrt()).to(self.lt.t.dtype))


class _CellModel(GruBasic):
    """Shared host side of the mini-batch `Lstm` / `Rnn` (poi_cell_step / poi_cell_predict, csrc/cells.hip): `train(idxs)` takes a LIST
    of users and makes ONE SGD step on the batch cost; predict / scoring / AUC / top-K are GruBasic's.  The tables are stored at the
    model's own dim: a sigmoid unit cannot be zero-padded (sigmoid(0) != 0)."""

    _pad_ok = False
    _cell = None            # _lib.CELL_RNN | _lib.CELL_LSTM
    _gates = ()             # leading axis of ui / wh / bi

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, **kw):
        if kw.get("table_dtype", "f32") != "f32":
            raise ValueError("%s stores float32 tables only (table_dtype=%r)" % (type(self).__name__, kw["table_dtype"]))
        init = dict(kw.pop("init", None) or {})
        own = {k: init.pop(k) for k in ("ui", "wh", "bi", "c0") if k in init}
        kw["pad_dim"] = False
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, init=init, **kw)
        D, g, seed = self.dim, self._gates, kw.get("seed")
        rng = np.random.default_rng(seed + 1) if seed is not None else np.random
        val = lambda k, shape, draw: np.asarray(own[k], np.float64).reshape(shape) if k in own else draw(shape)
        u = lambda shape: rng.uniform(-0.5, 0.5, shape)
        self.ui = Shared(self._dev(val("ui", g + (D, D), u)))                              # GRU.py:507 / :666
        self.wh = Shared(self._dev(val("wh", g + (D, D), u)))                              # :508 / :667
        self.bi = Shared(self._dev(val("bi", g + (D,), np.zeros)))                         # :510 / :668
        if self._cell == _lib.CELL_LSTM:
            self.c0 = Shared(self._dev(val("c0", (D,), np.zeros)))                         # :509 never trained
        self.params = [self.ui, self.wh, self.bi]                                          # :516 / :673
        self.l2 = _L2(self, ["lt", "ui", "wh", "bi"])                                      # :517-521 / :674-678

    def _cparams(self, snapshot=False):
        P = _lib.CellParams()
        P.lt = (self.trained_items if snapshot else self.lt).t.data_ptr()
        P.ui, P.wh, P.bi = self.ui.t.data_ptr(), self.wh.t.data_ptr(), self.bi.t.data_ptr()
        P.n_item, P.dim, P.cell = self.n_item, self.dim, self._cell
        return P

    def cell_session(self, n_slot=None):
        """Online state for this model (CellSession): per-slot h (and c) / last POI advanced one check-in at a time, top-K from it.
        (`session()` stays the GRU family's entry and refuses this class.)"""
        return CellSession(self, n_slot)

    def train(self, idxs):
        """seq_train(start_end) -> the batch's summed loss -upq (GRU.py:600, :755)."""
        return float(np.sum(self.train_batch(idxs), dtype=np.float64))

    def train_batch(self, idxs, sync=True):
        """One mini-batch step on the users `idxs` -> their losses (numpy, or the device tensor with sync=False).  An id out of range in
        the index tables raises IndexError and the launch moves nothing (checked with sync=True; the counter stays readable through
        ctx.take_bad_ids() otherwise)."""
        ids, _ = self._ids(idxs)
        n = ids.numel()
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        P, T = self._cparams(), self._tables()
        self.ctx.check(self.lib.poi_cell_step(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), n,
                                              self.alpha_lambda[0], self.alpha_lambda[1], _ptr(out), self._stream()))
        if not sync:
            return out
        bad = self.ctx.take_bad_ids(self._stream().value)
        if bad:
            raise IndexError("%d user(s) of the batch hold an id outside the tables: the launch moved nothing" % bad)
        return out.cpu().numpy()

    def predict_device(self, idxs):
        ids, out_row = self._by_length(idxs)
        n = ids.numel()
        hts = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        P, T = self._cparams(snapshot=True), self._tables()
        self.ctx.check(self.lib.poi_cell_predict(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), _ptr(out_row), n, _ptr(hts),
                                                 self._stream()))
        return hts


class Lstm(_CellModel):
    """public/GRU.py:502-657 - the mini-batch LSTM baseline: gates i, f, g, o, cell state c; ui, wh (4, D, D), bi (4, D), c0 (D)."""

    _cell = _lib.CELL_LSTM
    _gates = (4,)


class Rnn(_CellModel):
    """public/GRU.py:661-809 - the mini-batch sigmoid RNN baseline: h = sigmoid(ui x + wh h + bi); ui, wh (D, D), bi (D)."""

    _cell = _lib.CELL_RNN
    _gates = ()


class OboSpatialGru(GruBasic):
    """public/GRU_Spatial.py:42-292 - Distance2Pre."""

    spatial = True

    def __init__(self, train, test, dist, alpha_lambda, n_user, n_item, n_dists, n_in, n_hidden,
                 device="cuda:0", init=None, seed=None, coords=None, table_dtype="f32", pad_dim=True):
        n_dist, dd = n_dists
        self.n_dist, self.dd = int(n_dist), float(dd)                                      # dd in km (ref passes dd/1000)
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, device=device, init=init, seed=seed, table_dtype=table_dtype,
                         pad_dim=pad_dim)
        if self._csr is not None:
            dp, dq, tes_dist_masks = (np.ascontiguousarray(v, np.int32) for v in (self._csr.dp, self._csr.dq, self._csr.tes_dp))
        else:
            tra_dist_masks, tes_dist_masks, tra_dist_neg_masks = dist
            _, dp = padded_to_csr(tra_dist_masks, self._lens)
            _, dq = padded_to_csr(tra_dist_neg_masks, self._lens)
        self._check_ids("train distance bins", dp, self.n_dist); self._check_ids("negative distance bins", dq, self.n_dist)
        self._check_ids("test distance bins", tes_dist_masks, self.n_dist)
        self.dp, self.dq = torch.as_tensor(dp).to(self.device), torch.as_tensor(dq).to(self.device)
        self.tes_dist_masks = self._dev(tes_dist_masks, torch.int32)
        rng = np.random.default_rng(None if seed is None else seed + 1) if seed is not None else np.random
        u = lambda *s: rng.uniform(-0.5, 0.5, s)
        D, NB = self.dim, self.n_dist + 1
        init = init or {}
        g = lambda k, v: np.asarray(init[k], np.float64) if k in init else v()
        self.di = self._shared(g("di", lambda: u(NB, D)), "cols")                          # :57
        self.vs = self._shared(g("vs", lambda: u(NB, D)), "cols")                          # :60
        self.bs = Shared(self._dev(g("bs", lambda: np.zeros(NB))))                         # :61
        self.wd = Shared(self._dev(np.reshape(g("wd", lambda: rng.uniform(0, 0.5)), (1,))), scalar=True)   # :66
        self.loss_weight = Shared(self._dev(g("loss_weight", lambda: u(2))))               # :70
        self.trained_dists = self._shared(u(NB, D), "cols")                                # :74
        self.prob = None                       # dense (n_user, n_item) only on request (update_prob)
        self.trained_sus = None                # (n_user, NB) - fused alternative to `prob`
        self.use_bin_matrix = None             # None = auto: resident U x N bin matrix when it is <= 16 GiB, else bins on the fly
        self.coords = None if coords is None else self._dev(np.asarray(coords, np.float64), torch.float64)
        self._cphi = None if coords is None else self._dev(cos_lat(coords), torch.float64)
        self._binthr = None if coords is None else self._dev(bin_thresholds(self.dd * 1000.0, self.n_dist), torch.float64)
        self.params = [self.ui, self.wh, self.bi, self.vs, self.bs, self.wd, self.loss_weight]
        self.l2 = _L2(self, ["lt", "di", "ui", "wh", "bi", "vs", "bs", "wd", "loss_weight"])   # :83-88

    def _xw(self):
        return 2 * self.dim

    def load_params(self, loaded_objects):
        """public/GRU_Spatial.py:92-101: [loss_weight, wd, lt, di, ui, wh, bi, vs, bs]."""
        for sh, v in zip((self.loss_weight, self.wd, self.lt, self.di, self.ui, self.wh, self.bi, self.vs, self.bs), loaded_objects):
            sh.set_value(v)

    def s_update_neg_masks(self, tra_buys_neg_masks, tes_buys_neg_masks, tra_dist_neg_masks):
        """public/GRU_Spatial.py:103-107."""
        self.update_neg_masks(tra_buys_neg_masks, tes_buys_neg_masks)
        _, dq = padded_to_csr(tra_dist_neg_masks, self._lens)
        self.dq = torch.as_tensor(dq).to(self.device)

    def update_trained_dists(self):
        """public/GRU_Spatial.py:109-112."""
        self.trained_dists.t.copy_(self.di.t)

    def update_prob(self, prob):
        """public/GRU_Spatial.py:114-115 - dense (n_user, n_item) matrix (compatibility path)."""
        self.prob = self._dev(np.asarray(prob, np.float64)).reshape(self.n_user, self.n_item)

    def update_trained_sus(self, all_sus):
        """Fused replacement of fun_acquire_prob + update_prob (Load_Data_by_length.py:218-235): keep the
        (n_user, n_dist+1) distance-bin probabilities; prob rows are rebuilt on the device per batch
        from the POI coordinates (needs coords= at construction)."""
        t = all_sus if isinstance(all_sus, torch.Tensor) else self._dev(np.asarray(all_sus, np.float64))
        # rows padded to whole 32-user tiles (poi_score_topk_ulptai reads whole tiles); `trained_sus` is the
        # caller's table, `_sus_masked` the same with column n_dist ("too far") zeroed as the scoring path expects
        pad = ((self.n_user + 31) // 32) * 32
        buf = torch.zeros((pad, self.n_dist + 1), dtype=torch.float32, device=self.device)
        buf[:self.n_user] = t.to(self.device, torch.float32).reshape(self.n_user, self.n_dist + 1)
        self.trained_sus = buf[:self.n_user]
        self._sus_masked = buf.clone()
        self._sus_masked[:, self.n_dist] = 0.0
        self.prob = None
        lens = torch.as_tensor(self._off_host[1:].astype(np.int64) - 1).to(self.device)
        self._last_poi = self.p.index_select(0, lens).contiguous()

    def build_ulptai(self):
        """usrs_last_poi_to_all_intervals (prog_bpr_gru_spatial.py:90): distance bins of (last train POI,
        every POI), built once on the device and kept resident in the scoring kernel's tile order
        (include/poi_hip.h, poi_ulptai_build).  Needs coords= at construction."""
        if self.coords is None:
            raise _lib.PoiError("build_ulptai needs coords= at construction")
        bb = 1 if self.n_dist <= 255 else 2
        nut, nt = (self.n_user + 31) // 32, (self.n_item + 31) // 32
        lens = torch.as_tensor(self._off_host[1:].astype(np.int64) - 1).to(self.device)
        last = self.p.index_select(0, lens).contiguous()
        buf = torch.empty(nut * nt * 1024 * bb, dtype=torch.uint8, device=self.device)
        self.ctx.check(self.lib.poi_ulptai_build(self.ctx.handle, _ptr(self.coords), _ptr(self._cphi), _ptr(self._binthr), _ptr(last),
                                                 self.n_user, self.n_item, self.n_dist, self.dd * 1000.0, _ptr(buf), bb, self._stream()))
        self._ulptai, self._ulptai_bytes, self._ulptai_row = buf, bb, nt * 1024 * bb
        return buf

    def ulptai_host(self):
        """The (n_user, n_item) bin matrix decoded from the device layout (tests / inspection)."""
        buf = getattr(self, "_ulptai", None)
        if buf is None:
            buf = self.build_ulptai()
        bb = self._ulptai_bytes
        nut, nt = (self.n_user + 31) // 32, (self.n_item + 31) // 32
        a = buf.cpu().numpy().view(np.uint8 if bb == 1 else np.uint16).reshape(nut, nt, 64, 16)
        lane, r = np.arange(64)[:, None], np.arange(16)[None, :]
        row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)                 # (64, 16) user row within the tile
        col = np.broadcast_to(lane & 31, (64, 16))
        out = np.empty((nut * 32, nt * 32), np.int32)
        for ut in range(nut):
            blk = np.empty((32, nt, 32), np.int32)
            blk[row, :, col] = a[ut].transpose(1, 2, 0)
            out[ut * 32:(ut + 1) * 32] = blk.reshape(32, nt * 32)
        return out[:self.n_user, :self.n_item]

    def compute_sub_topk(self, start_end, k, return_scores=False):
        """Fused scoring + top-K.  With bin probabilities (update_trained_sus) and coordinates, contiguous
        user ranges starting at a multiple of 32 take the distance term from the resident bin matrix
        (poi_score_topk_ulptai); anything else falls back to the dense prob rows."""
        if k > 32:
            return self._topk_from_scores(start_end, k, return_scores)
        ids, lo = self._ids(start_end)
        ubm = self.use_bin_matrix
        if ubm is None:
            ubm = self.n_user * float(self.n_item) * (1 if self.n_dist <= 255 else 2) <= float(1 << 34)
        if ubm and self.prob is None and self.trained_sus is not None and self.coords is not None and lo is not None and lo % 32 == 0 \
                and self.kdim <= 128:
            if getattr(self, "_ulptai", None) is None:
                self.build_ulptai()
            n = ids.numel()
            users = self._rows(self.trained_users.t, ids, lo)
            st = self._sus_masked[lo:lo + n]
            idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
            sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
            bins = self._ulptai.data_ptr() + (lo // 32) * self._ulptai_row
            seed = self._seed_begin(lo, n, k)
            self.ctx.check(self.lib.poi_score_topk_ulptai(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), n, self.n_item, self.kdim,
                                                          _ptr(self.wd.t), _ptr(st), bins, self._ulptai_bytes, self.n_dist, int(k),
                                                          _ptr(idx), _ptr(sc), self._stream()))
            self._seed_end(seed, idx)
            return (idx, sc) if return_scores else idx
        if self.prob is None and self.trained_sus is not None and self.coords is not None:
            # anything else (unaligned / arbitrary id lists, dim 256, tables whose U x N bin matrix cannot exist): the bins are
            # computed on the fly inside the scoring kernel - no bin matrix, no dense prob rows
            return self._topk_geo(ids, lo, k, return_scores)
        return super().compute_sub_topk(start_end, k, return_scores)

    def _topk_geo(self, ids, lo, k, return_scores=False):
        n = ids.numel()
        users = self._rows(self.trained_users.t, ids, lo)
        pad = ((n + 31) // 32) * 32
        if lo is not None and lo + pad <= self._sus_masked.shape[0]:
            st = self._sus_masked[lo:lo + pad]
        else:                                   # whole 32-user tiles must be readable
            st = torch.zeros((pad, self.n_dist + 1), dtype=torch.float32, device=self.device)
            st[:n] = self._rows(self._sus_masked, ids, lo)
        lp = self._rows(self._last_poi, ids, lo)
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
        seed = self._seed_begin(lo, n, k)
        self.ctx.check(self.lib.poi_score_topk_geo(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), n, self.n_item, self.kdim, _ptr(self.wd.t),
                                                   _ptr(st), _ptr(self.coords), _ptr(self._cphi), _ptr(self._binthr), _ptr(lp), self.n_dist,
                                                   self.dd * 1000.0, int(k), _ptr(idx), _ptr(sc), self._stream()))
        self._seed_end(seed, idx)
        return (idx, sc) if return_scores else idx

    def _near_term(self, ids, lo):
        if self.prob is not None or self.trained_sus is None:
            raise _lib.PoiError("compute_sub_topk_near on the spatial model takes its distance term from the bin probabilities: "
                                "call update_trained_sus (a dense update_prob matrix is not covered)")
        return self.wd.t, self._rows(self._sus_masked, ids, lo), self._binthr, self.n_dist, self.dd * 1000.0

    def _rank_term(self, ids, lo):
        """The rows of sts and last train POI that _topk_geo ranks with; a model without bin probabilities ranks by the plain score, as
        its compute_sub_topk does."""
        if self.prob is not None:
            raise _lib.PoiError("compute_sub_target_rank on the spatial model takes its distance term from the bin probabilities: "
                                "call update_trained_sus (a dense update_prob matrix is not covered)")
        if self.trained_sus is None:
            return None
        if self.coords is None:
            raise _lib.PoiError("update_trained_sus needs coords= at construction")
        return self.wd.t, self._rows(self._sus_masked, ids, lo).contiguous(), self._rows(self._last_poi, ids, lo).contiguous()

    def _prob_rows(self, ids, lo):
        if self.prob is not None:
            return self.wd.t, self._rows(self.prob, ids, lo)
        if self.trained_sus is not None:
            if self.coords is None:
                raise _lib.PoiError("update_trained_sus needs coords= at construction")
            n = ids.numel()
            lp, st = self._rows(self._last_poi, ids, lo), self._rows(self.trained_sus, ids, lo)
            need = n * self.n_item                      # persistent grow-only buffer: no allocator churn per batch
            if getattr(self, "_prob_buf", None) is None or self._prob_buf.numel() < need:
                self._prob_buf = torch.empty(need, dtype=torch.float32, device=self.device)
            prob = self._prob_buf[:need].view(n, self.n_item)
            self.ctx.check(self.lib.poi_dist_prob(self.ctx.handle, _ptr(self.coords), _ptr(self._cphi), _ptr(self._binthr), _ptr(lp), _ptr(st), n,
                                                  self.n_item, self.n_dist, self.dd * 1000.0, _ptr(prob), self._stream()))
            return self.wd.t, prob
        return None, None

    def _params(self, snapshot=False):
        P = super()._params(snapshot)
        P.di = (self.trained_dists if snapshot else self.di).t.data_ptr()
        P.vs, P.bs, P.wd, P.lw = self.vs.t.data_ptr(), self.bs.t.data_ptr(), self.wd.t.data_ptr(), self.loss_weight.t.data_ptr()
        P.n_dist = self.n_dist
        return P

    def _tables(self):
        T = super()._tables()
        T.dp, T.dq = self.dp.data_ptr(), self.dq.data_ptr()
        return T

    def train(self, idx):
        """seq_train(uidx) -> [los, sur, upq, ls] (public/GRU_Spatial.py:222,290-292)."""
        o = self.train_batch(np.atleast_1d(idx))[0]
        return [float(o[0]), float(o[1]), float(o[2]), np.array([o[3], o[4]])]

    def train_batch(self, idxs, sync=True):
        """Throughput mode: (n, 5) rows [los, sur, upq, ls0, ls1]."""
        ids, _ = self._ids(idxs)
        n = ids.numel()
        out = torch.empty((n, 5), dtype=torch.float32, device=self.device)
        P, T = self._params(), self._tables()
        self.ctx.check(self.lib.poi_spatial_step(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), n,
                                                 self.alpha_lambda[0], self.alpha_lambda[1], _ptr(out), self._stream()))
        return out.cpu().numpy() if sync else out

    def train_sequence(self, idxs, sync=True):
        """The reference's epoch loop `for uidx in order: model.train(uidx)` (prog_bpr_gru_spatial.py:246-254) without a host round trip
        per step: the ids are staged on the device once and every user is ONE poi_spatial_step launch of one sequence (sequential SGD,
        the reference's semantics - not the batch rule), the (n, 5) loss rows [los, sur, upq, ls0, ls1] are read once at the end."""
        ids, _ = self._ids(idxs)
        n = ids.numel()
        out = torch.empty((n, 5), dtype=torch.float32, device=self.device)
        P, T = self._params(), self._tables()
        pP, pT, st = ctypes.byref(P), ctypes.byref(T), self._stream()
        ip, op = ids.data_ptr(), out.data_ptr()
        step, h, a, l = self.lib.poi_spatial_step, self.ctx.handle, self.alpha_lambda[0], self.alpha_lambda[1]
        for k in range(n):
            rc = step(h, pP, pT, ctypes.c_void_p(ip + 4 * k), 1, a, l, ctypes.c_void_p(op + 20 * k), st)
            if rc:
                self.ctx.check(rc)
        return out.cpu().numpy() if sync else out

    def predict(self, idxs):
        """public/GRU_Spatial.py:282-288 -> [hts (n, D), sts (n, n_dist+1)]."""
        h, s = self.predict_device(idxs)
        return [np.ascontiguousarray(h[:, :self.dim].cpu().numpy()), s.cpu().numpy()]

    def predict_device(self, idxs):
        ids, out_row = self._by_length(idxs)
        n = ids.numel()
        hts = torch.empty((n, self.kdim), dtype=torch.float32, device=self.device)
        sts = torch.empty((n, self.n_dist + 1), dtype=torch.float32, device=self.device)
        P, T = self._params(snapshot=True), self._tables()
        self.ctx.check(self.lib.poi_gru_predict(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), _ptr(out_row), n, _ptr(hts), _ptr(sts),
                                                self._stream()))
        return hts, sts


# =================================================================================================
class OboCARNN(GruBasic):
    """public/CA_RNN.py:46-227 - CA-RNN (flag 3 of prog_bpr_gru_spatial.py:141-151): interval-specific transition
    matrices wd[(n_dist+1), H, D], input matrix M (H, D), sigmoid RNN, BPR.  Same ctor as the reference; `ulptai` (the
    reference's U x N usrs_last_poi_to_all_intervals matrix) is accepted for signature compatibility but never
    uploaded: with coords= the scoring kernel computes those bins on the fly (bit-identical, tested)."""

    _near_ok = False

    spatial = True          # has distance-bin tables (negatives refresh computes dq)
    _pad_ok = False
    sync_names = ("lt", "wd", "M")      # every trainable tensor (dist.model_sync): POI table, interval matrices, input matrix

    def __init__(self, train, test, dist, alpha_lambda, n_user, n_item, n_dists, n_in, n_hidden, ulptai=None,
                 device="cuda:0", init=None, seed=None, coords=None):
        n_dist, dd = n_dists
        self.n_dist, self.dd = int(n_dist), float(dd)
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, device=device, init=init, seed=seed)
        if self._csr is not None:
            dp, dq, tes_dist_masks = (np.ascontiguousarray(v, np.int32) for v in (self._csr.dp, self._csr.dq, self._csr.tes_dp))
        else:
            tra_dist_masks, tes_dist_masks, tra_dist_neg_masks = dist
            _, dp = padded_to_csr(tra_dist_masks, self._lens)
            _, dq = padded_to_csr(tra_dist_neg_masks, self._lens)
        self._check_ids("train distance bins", dp, self.n_dist); self._check_ids("negative distance bins", dq, self.n_dist)
        self.dp, self.dq = torch.as_tensor(dp).to(self.device), torch.as_tensor(dq).to(self.device)
        self.tes_dist_masks = self._dev(tes_dist_masks, torch.int32)
        rng = np.random.default_rng(seed + 1) if seed is not None else np.random
        u = lambda *s: rng.uniform(-0.5, 0.5, s)
        D, NB = self.dim, self.n_dist + 1
        init = init or {}
        g = lambda k, v: np.asarray(init[k], np.float64) if k in init else v()
        self.M = Shared(self._dev(g("M", lambda: u(D, D))))                                # CA_RNN.py:55-56
        self.wd = Shared(self._dev(g("wd", lambda: u(NB, D, D))))                          # :61-62
        self.trained_dists = Shared(self._dev(u(NB, D, D)))                                # :66-67
        self.coords = None if coords is None else self._dev(np.asarray(coords, np.float64), torch.float64)
        self._cphi = None if coords is None else self._dev(cos_lat(coords), torch.float64)
        self._binthr = None if coords is None else self._dev(bin_thresholds(self.dd * 1000.0, self.n_dist), torch.float64)
        self.params = [self.M]
        self.l2 = _L2(self, ["lt", "wd", "M"])                                             # :70-76

    def s_update_neg_masks(self, tra_buys_neg_masks, tes_buys_neg_masks, tra_dist_neg_masks):
        """public/CA_RNN.py:80-84."""
        self.update_neg_masks(tra_buys_neg_masks, tes_buys_neg_masks)
        _, dq = padded_to_csr(tra_dist_neg_masks, self._lens)
        self.dq = torch.as_tensor(dq).to(self.device)

    def update_trained_dists(self):
        """public/CA_RNN.py:86-89."""
        self.trained_dists.t.copy_(self.wd.t)

    def _cparams(self, snapshot=False):
        P = _lib.CarnnParams()
        P.lt = (self.trained_items if snapshot else self.lt).t.data_ptr()
        P.wd = (self.trained_dists if snapshot else self.wd).t.data_ptr()
        P.M = self.M.t.data_ptr()
        P.n_item, P.n_dist, P.dim = self.n_item, self.n_dist, self.dim
        return P

    def _tables(self):
        T = super()._tables()
        T.dp, T.dq = self.dp.data_ptr(), self.dq.data_ptr()
        return T

    def cell_session(self, n_slot=None):
        """Online state for this model (CellSession): per-slot h / last POI advanced one check-in at a time by the literal predict step,
        ranked by compute_sub_all_scores' rule.  Needs coords= at construction.  (`session()` refuses this class.)"""
        return CellSession(self, n_slot)

    def train(self, idx):
        """seq_train(uidx) -> los (public/CA_RNN.py:160-170,219-221)."""
        return float(self.train_batch(np.atleast_1d(idx))[0])

    def train_batch(self, idxs, sync=True):
        ids, _ = self._ids(idxs)
        n = ids.numel()
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        P, T = self._cparams(), self._tables()
        self.ctx.check(self.lib.poi_carnn_step(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), n,
                                               self.alpha_lambda[0], self.alpha_lambda[1], _ptr(out), self._stream()))
        return out.cpu().numpy() if sync else out

    def predict_device(self, idxs):
        ids, _ = self._ids(idxs)
        n = ids.numel()
        hts = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        P, T = self._cparams(snapshot=True), self._tables()
        self.ctx.check(self.lib.poi_carnn_predict(self.ctx.handle, ctypes.byref(P), ctypes.byref(T), _ptr(ids), n, _ptr(hts), self._stream()))
        return hts

    def compute_sub_all_scores_device(self, start_end):
        """public/CA_RNN.py:91-101 -> (n, n_item) device tensor."""
        if self.coords is None:
            raise _lib.PoiError("OboCARNN scoring needs coords= at construction (the interval of (last train POI, POI) is computed on the device)")
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        if getattr(self, "_last_poi", None) is None:
            lens = torch.as_tensor(self._off_host[1:].astype(np.int64) - 1).to(self.device)
            self._last_poi = self.p.index_select(0, lens).contiguous()
        lp = self._rows(self._last_poi, ids, lo)
        out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_carnn_score_all(self.ctx.handle, _ptr(users), _ptr(self.trained_items.t), _ptr(self.M.t), _ptr(self.trained_dists.t),
                                                    _ptr(self.coords), _ptr(self._cphi), _ptr(self._binthr), _ptr(lp), n, self.n_item, self.n_dist,
                                                    self.dim, self.dd * 1000.0, _ptr(out), self._stream()))
        return out

    def compute_sub_topk(self, start_end, k, return_scores=False):
        """Valuate.py:132-146 on the CA-RNN scores: the (n, n_item) rows stay on the device, poi_topk selects."""
        return self._topk_from_scores(start_end, k, return_scores)

    _rank_fused = False


# =================================================================================================
class Explainer:
    """Leave-one-out attribution for the GRU family (OboSpatialGru, OboGru, Gru; include/poi_hip.h, poi_explain_loo): which past
    check-ins drove a recommendation.  `Explainer(model).explain(...)`; like a Session it reads the evaluation SNAPSHOTS trained_items /
    trained_dists as they are at the call and never changes a model parameter.  (A class of its own rather than a method of GruBasic:
    the recorded public signatures of the model classes - tests/golden/signatures.json - do not move.)"""

    EXPLAIN_C_MAX = 32
    EXPLAIN_WS_BYTES = 256 << 20      # of checkpoint states alive at a time: more rows go through the kernel in chunks

    def __init__(self, model):
        if not isinstance(model, GruBasic) or isinstance(model, (_CellModel, OboCARNN)):
            raise _lib.PoiError("explain covers the GRU family (OboSpatialGru, OboGru, Gru): %s is out of scope" % type(model).__name__)
        if model.spatial and model.coords is None:
            raise _lib.PoiError("explain on the spatial model needs coords= at construction")
        if model.kdim % 16 or not 16 <= model.kdim <= 256:
            raise _lib.PoiError("explain needs a stored dim that is a multiple of 16 in [16, 256] (got %d): build the model with pad_dim=True" % model.kdim)
        self.m = model

    def _explain_lists(self, lists, n):
        """lists -> (n, C <= 32) int32 device tensor; host lists are range-checked as nearest_visited checks them."""
        m = self.m
        if isinstance(lists, torch.Tensor) and lists.is_cuda:
            lt = lists.to(m.device, torch.int32)
        else:
            a = np.asarray(lists.cpu().numpy() if isinstance(lists, torch.Tensor) else lists).astype(np.int64)
            if a.size and (a.min() < -1 or a.max() >= m.n_item):
                raise IndexError("listed POIs must lie in [-1, %d) (found %d..%d)" % (m.n_item, int(a.min()), int(a.max())))
            lt = torch.as_tensor(a.astype(np.int32)).to(m.device)
        if lt.dim() != 2 or lt.shape[0] != n or not 1 <= lt.shape[1] <= self.EXPLAIN_C_MAX:
            raise ValueError("lists must be (%d rows, 1 <= C <= %d) (got %s)" % (n, self.EXPLAIN_C_MAX, tuple(lt.shape)))
        return lt.contiguous()

    def explain(self, start_end, lists, histories="train", by="checkin", return_states=False, sync=True):
        """WHY these POIs (include/poi_hip.h, poi_explain_loo): the leave-one-out attribution of listed POIs to a row's history.  For
        every row of start_end and every POI of its list - lists (n, C <= 32), -1 fill, typically the row's recommendations - the
        model's score with the whole history (base) and, per group g of the history, base minus the score with the group taken out
        (delta): positive - those check-ins pushed the POI up.  by="checkin": a group is one position; by="poi": every visit of one
        POI, groups in first-occurrence order.  The history without a group runs through the cell as a fresh session would, the step
        after a gap binned against the last kept POI; state, head and scores are float64.  histories: "train" (the rows' train
        sequences) or what fold_in takes (a CSR pair (off, p_flat), a list of sequences), one per row.
        Returns (base (n, C) float64, delta (G, C) float64, off (n + 1) int64: row r owns delta[off[r] : off[r + 1]], keys (G) int32:
        the POI every delta row removed) on the device[, dict(h (G, dim), sts (G, n_dist + 1) - spatial, last_poi (G)): the state of
        every variant].  A -1 entry gives NaN.  Host arguments are checked before the launch; device tensors by the kernel: a row
        with a POI out of range comes out NaN and - with sync - raises IndexError."""
        if by not in ("checkin", "poi"):
            raise ValueError("by must be 'checkin' or 'poi' (got %r)" % (by,))
        m = self.m
        ids, _ = m._ids(start_end)
        n = ids.numel()
        lt = self._explain_lists(lists, n)
        C = lt.shape[1]
        dev = m.device
        if isinstance(histories, str):
            if histories != "train":
                raise ValueError("histories must be 'train' or what fold_in takes (got %r)" % (histories,))
            off_h, ids_h = m._similar_train()[:2]
            a = ids.cpu().numpy().astype(np.int64)
            ln = off_h[a + 1] - off_h[a]
            o = np.concatenate(([0], np.cumsum(ln)))
            take = np.arange(int(o[-1])) - np.repeat(o[:-1] - off_h[a], ln)
            histories = (o, ids_h[take])
        on_device = isinstance(histories, tuple) and len(histories) == 2 and isinstance(histories[1], torch.Tensor) and histories[1].is_cuda
        off_t, p, n_h, total = m._foldin_csr(histories)
        if n_h != n:
            raise ValueError("explain: %d rows but %d histories" % (n, n_h))
        if not on_device and total and int(p[:total].max()) >= m.n_item:      # (fold_in admits the padding id n_item; a walk cannot)
            raise IndexError("history POIs must lie in [0, %d) (found %d)" % (m.n_item, int(p[:total].max())))
        off = off_t.cpu().numpy().astype(np.int64)
        lens = np.diff(off)
        if lens.size and lens.min() < 0:
            raise ValueError("histories=(off, p_flat): off must ascend")
        grp, g_off, keys, first, g_row = explain_groups(off_t.long(), p[:total], by)
        g_host = g_off.cpu().numpy()
        G = int(g_host[-1])
        base = torch.empty((n, C), dtype=torch.float64, device=dev)
        delta = torch.empty((G, C), dtype=torch.float64, device=dev)
        NB = m.n_dist + 1 if m.spatial else 0
        h_out = torch.empty((G, m.kdim), dtype=torch.float64, device=dev) if return_states else None
        s_out = torch.empty((G, NB), dtype=torch.float64, device=dev) if return_states and m.spatial else None
        l_out = torch.empty(G, dtype=torch.int32, device=dev) if return_states else None
        P, sp = m._params(snapshot=True), m.spatial
        mode = int(m.ctx.options.get("explain_start", 1))
        g32, lens_t = g_off.int().contiguous(), torch.as_tensor(lens).to(dev)
        grp = m._some_ids(grp.contiguous())
        per_row = max(1, (int(lens.max()) - 1) // 16 if n else 1) * m.kdim * 8
        for o, c in m._row_chunks(n, max(1, self.EXPLAIN_WS_BYTES // per_row)):
            g0, g1 = int(g_host[o]), int(g_host[o + c])
            bc, vc = explain_columns(lens_t[o:o + c], g_off[o:o + c + 1] - g0, first[g0:g1], g_row[g0:g1] - o, mode)
            m.ctx.check(m.lib.poi_explain_loo(
                m.ctx.handle, ctypes.byref(P), _ptr(m.coords if sp else None), _ptr(m._cphi if sp else None),
                _ptr(m._binthr if sp else None), m.dd * 1000.0 if sp else 0.0, _ptr(off_t[o:]), _ptr(p), total, _ptr(grp), _ptr(g32[o:]), G,
                c, int(lens[o:o + c].max()), _ptr(bc), _ptr(vc) if g1 > g0 else None, g1 - g0, _ptr(lt[o:]), C, _ptr(base[o:]), _ptr(delta),
                _ptr(h_out), _ptr(s_out), _ptr(l_out), m._stream()))
        states = None
        if return_states:
            states = dict(h=h_out[:, :m.dim], last_poi=l_out)
            if sp:
                states["sts"] = s_out
        return m._serve_out(base, ((delta, True), (g_off, True), (keys, True), (states, return_states)), sync and n > 0,
                               "row(s) with a history POI outside [0, %d) or a listed POI outside [-1, %d): their base, deltas and states are NaN"
                               % (m.n_item, m.n_item))


# =================================================================================================
class Session:
    """Online sessions of the GRU family (OboSpatialGru, OboGru, Gru): per-slot recurrent state on the device, advanced ONE check-in at a
    time (poi_session_advance, include/poi_hip.h) and ranked with the model's own scoring rule.  A slot holds h (kdim float64; `state`
    shows the logical dim), last_poi (-1: none yet), steps and - spatial - sts.  A fresh slot advanced through p[0 .. L-1] holds exactly
    what `predict` returns for a user whose training row is that sequence: every step reads the evaluation SNAPSHOTS trained_items /
    trained_dists as they are at the call, so a session follows update_trained_items() / update_trained_dists() and never changes a model
    parameter."""

    def __init__(self, model, n_slot=None):
        if not isinstance(model, GruBasic) or isinstance(model, (_CellModel, OboCARNN)):
            hint = " - use model.cell_session()" if isinstance(model, (_CellModel, OboCARNN)) else ""
            raise _lib.PoiError("Session covers the GRU family (OboSpatialGru, OboGru, Gru): %s is out of scope%s" % (type(model).__name__, hint))
        if model.spatial and model.coords is None:
            raise _lib.PoiError("session on the spatial model needs coords= at construction")
        self.m = m = model
        self.spatial = bool(model.spatial)
        self.n_slot = int(m.n_user if n_slot is None else n_slot)
        if self.n_slot <= 0:
            raise ValueError("n_slot must be positive")
        dev = m.device
        self.h = torch.zeros((self.n_slot, m.kdim), dtype=torch.float64, device=dev)
        self.last_poi = torch.full((self.n_slot,), -1, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(self.n_slot, dtype=torch.int32, device=dev)
        self.nb = m.n_dist + 1 if self.spatial else 0
        self.sts = torch.zeros((self.n_slot, self.nb), dtype=torch.float32, device=dev) if self.spatial else None

    # ---- ids ------------------------------------------------------------------------------------
    def _host_ids(self, name, ids, hi):
        a = np.atleast_1d(np.asarray(ids)).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= hi):
            raise IndexError("%s must lie in [0, %d) (found %d..%d)" % (name, hi, int(a.min()), int(a.max())))
        return a

    def _slot_tensor(self, slots):
        """int64 device tensor of slot ids (host ids are range-checked; slots=None: every slot)."""
        if slots is None:
            return torch.arange(self.n_slot, device=self.m.device)
        if isinstance(slots, torch.Tensor):
            return slots.to(self.m.device).long().reshape(-1)
        return torch.as_tensor(self._host_ids("slots", slots, self.n_slot)).to(self.m.device)

    def _i32(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.m.device)

    # ---- state ----------------------------------------------------------------------------------
    def reset(self, slots=None):
        """h = h0 = 0, last_poi = -1, steps = 0 (every slot, or the given ones)."""
        if slots is None:
            self.h.zero_(); self.last_poi.fill_(-1); self.steps.zero_()
            if self.spatial:
                self.sts.zero_()
            return
        ids = self._slot_tensor(slots)
        self.h[ids] = 0.0; self.last_poi[ids] = -1; self.steps[ids] = 0
        if self.spatial:
            self.sts[ids] = 0.0

    def load_history(self, users=None):
        """Seed slot u from user u's training row of the model's own tables: h and sts are the rows `predict_device` returns (what the
        evaluation path ranks with), last_poi the last train POI, steps the length."""
        m = self.m
        a = np.arange(m.n_user) if users is None else self._host_ids("users", users, min(m.n_user, self.n_slot))
        if a.size and a.max() >= self.n_slot:
            raise IndexError("users must lie in [0, %d): the session has that many slots" % self.n_slot)
        out = m.predict_device(a)
        ids = torch.as_tensor(a).to(m.device)
        hts, sts = out if self.spatial else (out, None)
        self.h[ids] = hts.double()
        last = torch.as_tensor(m._off_host[1:].astype(np.int64)[a] - 1).to(m.device)
        self.last_poi[ids] = m.p.index_select(0, last)
        self.steps[ids] = torch.as_tensor(np.asarray(m._lens)[a].astype(np.int32)).to(m.device)
        if self.spatial:
            self.sts[ids] = sts

    def seed(self, slots, h, last_poi, steps=None):
        """State from outside (a checkpoint, another model's rows): h (n, dim) or (n, kdim), last_poi (n) with -1 = none; sts is
        recomputed through the head (poi_session_sts)."""
        m = self.m
        ids = self._slot_tensor(slots)
        n = ids.numel()
        ht = h if isinstance(h, torch.Tensor) else torch.as_tensor(np.asarray(h, np.float64))
        self.h[ids] = m._pad_cols(ht.to(m.device, torch.float64).reshape(n, -1))
        lp = self._host_ids("last_poi + 1", np.asarray(last_poi, np.int64) + 1, m.n_item + 1) - 1
        self.last_poi[ids] = self._i32(lp)
        self.steps[ids] = self._i32(np.zeros(n) if steps is None else steps)
        if self.spatial and n:
            P = m._params(snapshot=True)
            out = torch.empty((n, self.nb), dtype=torch.float32, device=m.device)
            sl = ids.int().contiguous()
            m.ctx.check(m.lib.poi_session_sts(m.ctx.handle, ctypes.byref(P), _ptr(self.h), self.n_slot, _ptr(sl), n, _ptr(out), m._stream()))
            self.sts[ids] = out

    def state(self, slots=None):
        """Host copies at the logical dim: dict(h (n, dim) float64, last_poi, steps[, sts])."""
        ids = self._slot_tensor(slots)
        out = dict(h=np.ascontiguousarray(self.h.index_select(0, ids)[:, :self.m.dim].cpu().numpy()),
                   last_poi=self.last_poi.index_select(0, ids).cpu().numpy(), steps=self.steps.index_select(0, ids).cpu().numpy())
        if self.spatial:
            out["sts"] = self.sts.index_select(0, ids).cpu().numpy()
        return out

    # ---- advance --------------------------------------------------------------------------------
    def _launch(self, slot_ptr, poi_ptr, n, hts_out=None, sts_out=None):
        m = self.m
        P = m._params(snapshot=True)
        sp = self.spatial
        m.ctx.check(m.lib.poi_session_advance(m.ctx.handle, ctypes.byref(P), _ptr(m.coords if sp else None), _ptr(m._cphi if sp else None),
                                              _ptr(m._binthr if sp else None), m.dd * 1000.0 if sp else 0.0, _ptr(self.h), _ptr(self.sts),
                                              _ptr(self.last_poi), _ptr(self.steps), self.n_slot, ctypes.c_void_p(slot_ptr),
                                              ctypes.c_void_p(poi_ptr), int(n), _ptr(hts_out), _ptr(sts_out), m._stream()))

    def _raise_bad(self):
        bad = self.m.ctx.take_bad_ids(self.m._stream().value)
        if bad:
            raise IndexError("%d event(s) named a slot outside [0, %d), a POI outside [0, %d) or - in a device batch - a slot more than once: "
                             "those slots were left untouched" % (bad, self.n_slot, self.m.n_item))

    def advance(self, slots, pois, sync=True, return_state=False):
        """Apply the check-ins (slots[i], pois[i]).  Host arrays are range-checked first (IndexError, nothing moves) and may name a slot
        several times: the batch is split into successive launches that keep each slot's order.  Device tensors are one launch and are
        checked by the kernel: a bad id or a repeated slot leaves that slot untouched and raises IndexError (with sync=True; otherwise
        the count stays readable through ctx.take_bad_ids()).  return_state: (hts (n, kdim)[, sts (n, n_dist + 1)]) float32 device rows
        of the new state, in the order of the call."""
        m = self.m
        dev_in = isinstance(slots, torch.Tensor) or isinstance(pois, torch.Tensor)
        if dev_in:
            st = slots if isinstance(slots, torch.Tensor) else self._i32(self._host_ids("slots", slots, self.n_slot))
            pt = pois if isinstance(pois, torch.Tensor) else self._i32(self._host_ids("pois", pois, m.n_item))
            st = st.to(m.device, torch.int32).contiguous().reshape(-1); pt = pt.to(m.device, torch.int32).contiguous().reshape(-1)
            rounds = [None]
        else:
            s = self._host_ids("slots", slots, self.n_slot)
            j = self._host_ids("pois", pois, m.n_item)
            st, pt = self._i32(s), self._i32(j)
            rounds = [None]
            if len(s) > 1 and len(np.unique(s)) < len(s):
                order = np.argsort(s, kind="stable")
                ss, pos = s[order], np.arange(len(s))
                first = np.maximum.accumulate(np.where(np.r_[True, ss[1:] != ss[:-1]], pos, 0))
                rank = np.empty(len(s), np.int64)
                rank[order] = pos - first                     # occurrence number of the event within its slot
                rounds = [np.nonzero(rank == r)[0] for r in range(int(rank.max()) + 1)]
        if st.numel() != pt.numel():
            raise ValueError("slots and pois must have the same length (%d vs %d)" % (st.numel(), pt.numel()))
        n = st.numel()
        hts = torch.empty((n, m.kdim), dtype=torch.float32, device=m.device) if return_state else None
        sts = torch.empty((n, self.nb), dtype=torch.float32, device=m.device) if return_state and self.spatial else None
        for sel in rounds:
            if sel is None:
                self._launch(st.data_ptr(), pt.data_ptr(), n, hts, sts)
                continue
            it = torch.as_tensor(sel).to(m.device)
            s_r, p_r = st.index_select(0, it), pt.index_select(0, it)
            h_r = torch.empty((len(sel), m.kdim), dtype=torch.float32, device=m.device) if return_state else None
            t_r = torch.empty((len(sel), self.nb), dtype=torch.float32, device=m.device) if sts is not None else None
            self._launch(s_r.data_ptr(), p_r.data_ptr(), len(sel), h_r, t_r)
            if return_state:
                hts[it] = h_r
                if sts is not None:
                    sts[it] = t_r
        if sync:
            self._raise_bad()
        if return_state:
            return (hts, sts) if self.spatial else hts

    def replay(self, off, p_flat, slots=None, sync=True):
        """Advance through CSR sequences (the layout of data.padded_to_csr): sequence k = p_flat[off[k] : off[k + 1]] goes to slots[k]
        (default k).  The events are laid out step-major on the device once; launch t then carries the slots whose sequence is longer
        than t, straight from that layout - no host round trip per step beyond the launch."""
        m = self.m
        off = np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off, np.int64)
        p = np.asarray(p_flat.cpu() if isinstance(p_flat, torch.Tensor) else p_flat, np.int64)
        lens = np.diff(off)
        nseq = len(lens)
        sl = np.arange(nseq) if slots is None else np.atleast_1d(np.asarray(slots)).astype(np.int64)
        if len(sl) != nseq:
            raise ValueError("replay: %d sequences but %d slots" % (nseq, len(sl)))
        self._host_ids("slots", sl, self.n_slot)
        if len(np.unique(sl)) != nseq:
            raise ValueError("replay: every sequence needs a slot of its own")
        if nseq == 0 or lens.max() <= 0:
            return
        self._host_ids("pois", p[off[0]:off[-1]], m.n_item)
        order = np.argsort(-lens, kind="stable")
        lo, so, st0 = lens[order], sl[order], off[:-1][order]
        L = int(lo[0])
        cnt = [int(np.searchsorted(-lo, -t, side="left")) for t in range(L)]      # sequences longer than t (lo is descending)
        s_sm = np.concatenate([so[:c] for c in cnt])
        p_sm = np.concatenate([p[st0[:c] + t] for t, c in enumerate(cnt)])
        sd, pd = self._i32(s_sm), self._i32(p_sm)
        pos = 0
        for c in cnt:
            self._launch(sd.data_ptr() + 4 * pos, pd.data_ptr() + 4 * pos, c)
            pos += c
        if sync:
            self._raise_bad()

    # ---- recommend ------------------------------------------------------------------------------
    # Every serving call below is "make the slots' ScoreSource, call the model's family function".  A CellSession of Lstm / Rnn ranks by
    # the plain rule, as a session of the plain GRU does.  A CA-RNN CellSession ranks by its own score rows (CellSession._carnn_rows):
    # a slot without a check-in has no scorable POI and gives -1 ids (NaN scores from recommend / rank_of, count 0, labels -1 with
    # log-probability -inf, list scores -inf), and what needs users . items is refused (CellSession._refusals).
    def _need_fused(self, family):
        """Group, audience and route do not rank one score row per slot: they take users . items from the slots' fused source and
        refuse a session whose rows are not fused before anything is looked at.  These sessions' rows always are; CellSession's may
        not be."""

    def _source(self, slots):
        """The fused ScoreSource of the slots' CURRENT states: users = h as float32, the anchor = last_poi (-1: no check-in yet), and
        - spatial - the distance term of the slots' sts rows.  tile_term: a slot without a check-in has no term - its sts row is zero,
        and so is column n_dist ("too far") of every row; the last POI rows are the slots' own (the kernels read -1 as "no term")
        unless clamped to 0.  near_term: the sts rows as they are; the kernels skip the term of an anchor -1 themselves."""
        m = self.m
        ids = self._slot_tensor(slots)
        n = ids.numel()
        users = self.h.index_select(0, ids).float().contiguous()
        lpr = self.last_poi.index_select(0, ids).contiguous()

        def tile_term(clamp, pad):
            if not self.spatial:
                return None
            st = torch.zeros((((n + 31) // 32) * 32 if pad else n, self.nb), dtype=torch.float32, device=m.device)
            st[:n] = self.sts.index_select(0, ids) * (lpr >= 0).float()[:, None]
            st[:, m.n_dist] = 0.0
            return m.wd.t, st, lpr.clamp(min=0).contiguous() if clamp else lpr

        def near_term():
            return (m.wd.t, self.sts.index_select(0, ids).contiguous(), m._binthr, m.n_dist, m.dd * 1000.0) if self.spatial else None
        return ScoreSource(m, n, ("last",), lambda: lpr, None, users=users, items=m.trained_items.t, tile_term=tile_term, near_term=near_term)

    def recommend(self, slots, k, return_scores=False, within_km=None, exclude=None, return_counts=False, sync=True):
        """(n, k) int32 device indices by descending score, ties by ascending index: h . trained_items[:-1]^T, plus - spatial -
        wd * sts[bin(last_poi, .)] for bins below n_dist.  A slot without a check-in has no distance term.
        within_km / exclude / return_counts rank over restricted candidates instead (poi_score_topk_near, k <= 32): the POIs within
        within_km km of the slot's last_poi (a slot without a check-in ignores the radius), minus exclude = "last" (the last_poi) or CSR
        lists (off, ids); -1 ids where fewer than k candidates remain.  Plain models need set_coords() for a radius.  The defaults
        keep the unrestricted path.  CA-RNN: compute_sub_all_scores' rule on the slots' CURRENT h and last_poi (explicit score rows,
        <= 1 GiB at a time, + poi_topk, k <= 64); within_km / exclude / return_counts are not defined for its score rule and raise."""
        m = self.m
        src = self._source(slots)
        n, k = src.n, int(k)
        if within_km is not None or exclude is not None or return_counts:
            return m._serve_near(src, k, within_km, exclude, None, return_scores, return_counts, sync)
        if not src.fused:
            return src.finish(m._topk_from_rows(src.score_rows(), n, k, return_scores), return_scores, False, ranked=True)
        users = src.users
        wd, st, lp = src.tile_term(clamp=True, pad=True) or (None, None, None)
        if k <= 32:
            idx, sc, _ = m._topk_buffers(n, k, return_scores, False)
            if self.spatial:
                m.ctx.check(m.lib.poi_score_topk_geo(m.ctx.handle, _ptr(users), _ptr(m.trained_items.t), n, m.n_item, m.kdim, _ptr(wd), _ptr(st),
                                                     _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), _ptr(lp), m.n_dist, m.dd * 1000.0, k,
                                                     _ptr(idx), _ptr(sc), m._stream()))
            else:
                m.ctx.check(m.lib.poi_score_topk(m.ctx.handle, _ptr(users), _ptr(m.trained_items.t), n, m.n_item, m.kdim, None, None, k,
                                                 _ptr(idx), _ptr(sc), m._stream()))
            return (idx, sc) if return_scores else idx

        def score_rows(o, c):
            prob = None
            if self.spatial:
                prob = torch.empty((c, m.n_item), dtype=torch.float32, device=m.device)
                m.ctx.check(m.lib.poi_dist_prob(m.ctx.handle, _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), _ptr(lp[o:o + c]), _ptr(st[o:o + c]), c,
                                                m.n_item, m.n_dist, m.dd * 1000.0, _ptr(prob), m._stream()))
            full = torch.empty((c, m.n_item), dtype=torch.float32, device=m.device)
            m.ctx.check(m.lib.poi_score_all(m.ctx.handle, _ptr(users[o:o + c]), _ptr(m.trained_items.t), c, m.n_item, m.kdim, _ptr(wd), _ptr(prob),
                                            _ptr(full), m._stream()))
            return full
        return m._topk_from_rows(score_rows, n, k, return_scores)

    def recommend_filtered(self, slots, k, filt, which=None, within_km=None, exclude=None, path="auto", return_scores=False, return_counts=False,
                           sync=True):
        """model.compute_sub_topk_filtered over the slots' CURRENT states: the top-k (k <= 32) among the POIs that pass a predicate of
        `filt` (which: the predicate index of every slot, default predicate 0), the slot's last_poi as the anchor of the radius and of
        the spatial distance term (a slot without a check-in has neither).  exclude: None, "last" or CSR lists (off, ids).  CA-RNN: its
        own score rows + poi_topk_filtered_scores; within_km is not defined for its score rule."""
        return self.m._serve_filtered(self._source(slots), k, filt, which, within_km, exclude, None, path, return_scores, return_counts, sync)

    def recommend_capped(self, slots, k, labels, per=1, filt=None, which=None, exclude=None, return_scores=False, return_labels=False,
                         return_counts=False, sync=True):
        """model.compute_sub_topk_capped over the slots' CURRENT states (h, sts, last_poi, as `candidates` assembles them): the top-k
        (k <= 32) with at most `per` POIs of one label of `labels` (a PoiLabels).  exclude: None, "last" or CSR lists (off, ids).  A
        slot without a check-in has no distance term.  CA-RNN: its own score rows + poi_topk_capped_scores."""
        return self.m._serve_capped(self._source(slots), k, labels, per, filt, which, exclude, return_scores, return_labels, return_counts, sync)

    def recommend_labels(self, slots, k, labels, by="mass", exclude=None, return_best=False, sync=True):
        """model.recommend_labels over the slots' CURRENT states (h, sts, last_poi, as `candidates` assembles them): the k (<= 32) labels
        of `labels` (a PoiLabels) the next check-in most likely falls in, by softmax mass (by="mass") or by the label's best POI
        (by="max"), with their log-probabilities.  exclude: None, "last" or CSR lists (off, ids).  A slot without a check-in has no
        distance term.  CA-RNN: its own score rows + poi_labels_scores."""
        return self.m._serve_labels(self._source(slots), k, labels, by, exclude, return_best, sync)

    def rank_of(self, slots, pois, exclude=None, return_scores=False, return_counts=False, sync=True):
        """Exact 0-based rank of pois[i] (one POI per slot, or (n, len_t <= 8)) among all POIs under the slot's CURRENT state - the score
        rule of `recommend` (h . trained_items[:-1]^T, plus the spatial distance term at last_poi; none before the first check-in):
        model.compute_sub_target_rank through the session's h / sts / last_poi.  exclude: None, "last" or CSR lists (off, ids).  CA-RNN
        goes through its score rows and poi_rank_scores; a slot without a check-in gives rank -1 (NaN score, count 0)."""
        src = self._source(slots)
        pois = pois.reshape(src.n, -1) if isinstance(pois, torch.Tensor) else np.asarray(pois).reshape(src.n, -1)
        return self.m._serve_rank(src, pois, exclude, return_scores, return_counts, sync)

    def candidates(self, slots, k, exclude=None, return_scores=False, return_counts=False, sync=True):
        """model.compute_sub_candidates over the slots' CURRENT states (h, sts, last_poi, as `rank_of` assembles them): the exact top-k
        of every slot for 1 <= k <= min(4096, n_item).  exclude: None, "last" or CSR lists (off, ids).  A slot without a check-in has no
        distance term.  CA-RNN: its own score rows + poi_topk_select."""
        return self.m._serve_candidates(self._source(slots), k, exclude, return_scores, return_counts, sync)

    def score_lists(self, slots, lists, sync=True):
        """model.score_lists over the slots' CURRENT states (h, sts, last_poi, as `candidates` assembles them): the scores of explicit
        candidate lists.  A slot without a check-in has no distance term.  CA-RNN: the listed columns of its own score rows."""
        return self.m._serve_score_lists(self._source(slots), lists, sync)

    def rerank(self, slots, lists, k, prior=None, weights=(1.0, 0.0), return_scores=False, return_positions=False, return_counts=False, sync=True):
        """model.rerank over the slots' CURRENT states: every slot's candidate list scored under its state and returned in order
        (k <= 4096; optionally blended with a prior).  CA-RNN: its own score rows, a gather of the listed columns and
        poi_rerank_lists."""
        return self.m._serve_rerank(self._source(slots), lists, k, prior, weights, return_scores, return_positions, return_counts, sync)

    def recommend_diverse(self, slots, k, pool=64, trade=0.7, geo_weight=1.0, scale_km=1.0, exclude=None, return_scores=False,
                          return_objective=False, return_pool=False, return_counts=False, sync=True):
        """model.compute_sub_topk_diverse over the slots' CURRENT states (h, sts, last_poi, as `rank_of` assembles them): the `pool`
        best POIs of every slot, re-ranked for relevance against redundancy.  exclude: None, "last" or CSR lists (off, ids).  A slot
        without a check-in has no distance term.  CA-RNN: its own score rows, the exclusions masked, the pool from poi_topk, then
        poi_diverse_rerank."""
        return self.m._serve_diverse(self._source(slots), k, pool, trade, geo_weight, scale_km, exclude, return_scores, return_objective, return_pool,
                                     return_counts, sync)

    def recommend_group(self, slot_groups, k, agg="mean", exclude=None, return_scores=False, return_counts=False, sync=True):
        """model.recommend_group over the slots' CURRENT states (h, sts, last_poi, as `rank_of` assembles them): slot_groups is a list of
        lists of slot ids or a CSR pair (off, ids); agg "mean" or "min"; exclude None or CSR lists (off, ids), one per group.  A slot
        without a check-in has no distance term.  CA-RNN ranks by a rule of its own and is refused."""
        self._need_fused("group")
        m = self.m
        k, agg = m._group_args(k, agg)
        off, ids, on_device = m._group_csr(slot_groups, self.n_slot, "slot_groups")
        n_grp = len(off) - 1
        if n_grp == 0:
            return m._group_out(*m._topk_buffers(0, k, True, True), return_scores, return_counts, False)
        ex = m._group_exclusion(exclude, off, ids, n_grp, kinds=())
        uniq, mem = m._group_members(ids, self.n_slot)
        src = self._source(torch.as_tensor(uniq).to(m.device))
        return m._group_launch(src.users, src.items, src.tile_term() if len(uniq) else None, self._i32(off), m._some_ids(self._i32(mem)), n_grp, agg,
                               ex, k, return_scores, return_counts, sync)

    def audience(self, pois, k, slots=None, exclude=None, return_scores=False, return_counts=False, sync=True):
        """model.recommend_audience over the slots' CURRENT states (h, sts, last_poi, as `candidates` assembles them): which live
        sessions should hear about this POI?  slots: None = every slot, or an ascending unique list of slot ids.  exclude: None or a
        CSR pair (off, ids) of slot ids per query.  Returns (n_q, k) int32 SLOT ids by descending score, ties by ascending id, -1 fill
        [, scores][, candidate counts].  A slot without a check-in has no distance term.  CA-RNN ranks by a rule of its own and is
        refused."""
        self._need_fused("audience")
        m = self.m
        seg = m._audience_segment(slots, self.n_slot, "slots")
        n = self.n_slot if seg is None else len(seg)
        k = m._audience_k(k, n, True)
        q = m._audience_queries(pois)
        ex = m._audience_exclusion(exclude, q, seg, self.n_slot, kinds=())
        src = self._source(seg)
        return m._audience_launch(src.users, src.items, m.kdim, src.tile_term() if n else None, q, ex, k, None if seg is None else self._i32(seg),
                                  return_scores, return_counts, sync)

    # ---- routes ---------------------------------------------------------------------------------
    ROUTE_BEAM_MAX, ROUTE_STEPS_MAX = 8, 16

    @classmethod
    def _route_args(cls, steps, beam):
        steps, beam = int(steps), int(beam)
        if not 1 <= beam <= cls.ROUTE_BEAM_MAX:
            raise _lib.PoiError("route recommendation supports 1 <= beam <= %d (got %d)" % (cls.ROUTE_BEAM_MAX, beam))
        if not 1 <= steps <= cls.ROUTE_STEPS_MAX:
            raise _lib.PoiError("route recommendation supports 1 <= steps <= %d (got %d)" % (cls.ROUTE_STEPS_MAX, steps))
        return steps, beam

    def _route_expand(self, users, sts, last_poi, path, path_len, ex, rows_per_list, live, b, return_counts=False):
        """One poi_route_expand call on explicit rows -> (idx (n, b), score (n, b), lse (n) float64[, counts]) device tensors.  sts /
        last_poi: the rows' distance-term state (spatial sessions) or None."""
        m = self.m
        n = users.shape[0]
        idx = torch.empty((n, b), dtype=torch.int32, device=m.device)
        sc = torch.empty((n, b), dtype=torch.float32, device=m.device)
        lse = torch.empty(n, dtype=torch.float64, device=m.device)
        cnt = torch.empty(n, dtype=torch.int32, device=m.device) if return_counts else None
        term = (m.wd.t, sts, last_poi) if sts is not None else None
        m.ctx.check(m.lib.poi_route_expand(m.ctx.handle, *m._tile_operands(users, m.trained_items.t, users.shape[1], term), _ptr(path),
                                           path.shape[1] if path is not None else 0, int(path_len), _ptr(ex[0]), _ptr(ex[1]), int(rows_per_list), _ptr(live),
                                           int(b), _ptr(idx), _ptr(sc), _ptr(lse), _ptr(cnt), m._stream()))
        return (idx, sc, lse, cnt) if return_counts else (idx, sc, lse)

    def _route_merge(self, idx, sc, lse, total, n_live, n_slot, n_par, b, return_step_scores=False):
        """One poi_route_merge call -> (parent, poi, total (n_slot, b), steplp | None, n_live (n_slot)) device tensors."""
        m = self.m
        parent = torch.empty((n_slot, b), dtype=torch.int32, device=m.device)
        poi = torch.empty((n_slot, b), dtype=torch.int32, device=m.device)
        tot = torch.empty((n_slot, b), dtype=torch.float64, device=m.device)
        slp = torch.empty((n_slot, b), dtype=torch.float64, device=m.device) if return_step_scores else None
        nl = torch.empty(n_slot, dtype=torch.int32, device=m.device)
        m.ctx.check(m.lib.poi_route_merge(m.ctx.handle, _ptr(idx), _ptr(sc), _ptr(lse), _ptr(total), _ptr(n_live), n_slot, n_par, b, _ptr(parent), _ptr(poi),
                                          _ptr(tot), _ptr(slp), _ptr(nl), m._stream()))
        return parent, poi, tot, slp, nl

    _ROUTE_STATE = ("h", "c", "sts", "last_poi", "steps")      # what a hypothesis inherits from its parent (c: an Lstm's cell state)

    def recommend_route(self, slots, steps, beam=4, exclude="last", revisit=False, return_step_scores=False, sync=True):
        """The best `beam` routes of `steps` next POIs for every slot under its CURRENT state (include/poi_hip.h, route recommendation):
        a beam search whose step score is the log-softmax over all POIs of the score rule of `recommend`.  At every step each live
        hypothesis proposes its best `beam` POIs outside exclude and - unless revisit - outside its own path (poi_route_expand), the
        slot keeps the best `beam` of the proposals by total log-probability (poi_route_merge), and the survivors are advanced by their
        POI on a scratch session of n * beam slots.  exclude: None, "last" (the slot's last_poi at the call) or CSR lists (off, ids) per
        slot.  Returns paths (n, beam, steps) int32 and logp (n, beam) float64 device tensors, beams by descending logp (-1 / -inf: a
        dead beam - fewer candidates than beams); with return_step_scores also the per-step log-probabilities (n, beam, steps) float64.
        The session's own slots are only read (they may repeat): a route is a what-if.  The loop issues no host synchronisation;
        sync=True raises IndexError at the end when a device exclusion list was malformed.  CA-RNN ranks by a rule of its own and is
        refused."""
        self._need_fused("route")
        m = self.m
        T, B = self._route_args(steps, beam)
        ids = self._slot_tensor(slots)
        n = ids.numel()
        dev = m.device
        paths = torch.full((n * B, T), -1, dtype=torch.int32, device=dev)
        total = torch.zeros((n, 1), dtype=torch.float64, device=dev)
        slp = torch.full((n * B, T), float("-inf"), dtype=torch.float64, device=dev) if return_step_scores else None
        if n == 0:
            out = (paths.view(0, B, T), total.new_zeros((0, B)))
            return out + (slp.view(0, B, T),) if return_step_scores else out
        src = {k: getattr(self, k).index_select(0, ids) for k in self._ROUTE_STATE if getattr(self, k, None) is not None}
        ex = m._near_exclusion(exclude, n, src["last_poi"].contiguous(), kinds=("last",))      # (the rows are in hand: no source)
        scratch = type(self)(m, n_slot=n * B)
        all_rows = torch.arange(n * B, dtype=torch.int32, device=dev)
        base = torch.arange(n, device=dev)[:, None]
        beam_no = torch.arange(B, dtype=torch.int32, device=dev)[None, :]
        P, nlive, live = 1, None, None
        for t in range(T):
            users = src["h"].float().contiguous()
            sts = src["sts"].contiguous() if self.spatial else None
            lp = src["last_poi"].contiguous() if self.spatial else None
            idx, sc, lse = self._route_expand(users, sts, lp, None if revisit or t == 0 else paths, 0 if revisit else t, ex, P, live, B)
            parent, poi, total, step_lp, nlive = self._route_merge(idx, sc, lse, total, nlive, n, P, B, return_step_scores)
            flat = (base * P + parent.long()).reshape(-1)
            if t > 0:
                paths = paths.index_select(0, flat)
            paths[:, t] = poi.reshape(-1)
            if slp is not None:
                if t > 0:
                    slp = slp.index_select(0, flat)
                slp[:, t] = step_lp.reshape(-1)
            if t + 1 == T:
                break
            for k in src:                                # the survivors' states, then one check-in each (a dead row: POI 0, it stays dead)
                setattr(scratch, k, src[k].index_select(0, flat).contiguous())
            nxt = poi.clamp(min=0).reshape(-1).contiguous()
            scratch._launch(all_rows.data_ptr(), nxt.data_ptr(), n * B)
            src = {k: getattr(scratch, k) for k in src}
            live = (beam_no < nlive[:, None]).int().contiguous()
            P = B
        if sync:
            bad = m.ctx.take_bad_ids(m._stream().value)
            if bad:
                raise IndexError("%d hypothesis row(s) with an exclusion id outside [0, %d) or a list that is not ascending: their routes are dead" % (bad, m.n_item))
        out = (paths.view(n, B, T), total)
        return out + (slp.view(n, B, T),) if return_step_scores else out


class CellSession(Session):
    """Online sessions of the baselines `Lstm`, `Rnn` and `OboCARNN` (model.cell_session()): the slot bookkeeping, `advance`, `replay`
    and the repeated-slot rule of `Session` over the cell steps of poi_session_cell_advance / poi_session_carnn_advance
    (include/poi_hip.h).  A slot holds h (dim float64), c (Lstm only), last_poi (-1: none yet) and steps; there is no sts.  A fresh slot
    advanced through p[0 .. L-1] holds what `predict` returns for a user whose training row is that sequence; every step reads the
    evaluation snapshots as they are at the call (trained_items, and trained_dists for CA-RNN) and never changes a model parameter.
    Lstm and Rnn rank as the plain GRU session does (h . trained_items[:-1]^T; within_km / exclude / return_counts after set_coords()).
    CA-RNN ranks by its own rule (poi_carnn_score_all on the slots' h and last_poi + poi_topk / poi_rank_scores): a slot without a
    check-in has no last POI and gets index -1 / a NaN score / rank -1, and within_km is refused as on the model itself."""

    def __init__(self, model, n_slot=None):
        if not isinstance(model, (_CellModel, OboCARNN)):
            raise _lib.PoiError("CellSession covers Lstm, Rnn and OboCARNN: use model.session() for %s" % type(model).__name__)
        self.carnn = isinstance(model, OboCARNN)
        if self.carnn and model.coords is None:
            raise _lib.PoiError("cell_session on OboCARNN needs coords= at construction (the interval of a check-in is computed on the device)")
        self.m = m = model
        self.lstm = not self.carnn and m._cell == _lib.CELL_LSTM
        self.spatial = False                        # no sts and no distance term: the plain paths of Session
        self.n_slot = int(m.n_user if n_slot is None else n_slot)
        if self.n_slot <= 0:
            raise ValueError("n_slot must be positive")
        dev = m.device
        self.h = torch.zeros((self.n_slot, m.dim), dtype=torch.float64, device=dev)
        self.c = torch.zeros((self.n_slot, m.dim), dtype=torch.float64, device=dev) if self.lstm else None
        self.last_poi = torch.full((self.n_slot,), -1, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(self.n_slot, dtype=torch.int32, device=dev)
        self.nb, self.sts = 0, None

    # ---- state ----------------------------------------------------------------------------------
    def reset(self, slots=None):
        """h = c = 0, last_poi = -1, steps = 0 (every slot, or the given ones)."""
        super().reset(slots)
        if self.lstm:
            if slots is None:
                self.c.zero_()
            else:
                self.c[self._slot_tensor(slots)] = 0.0

    def load_history(self, users=None):
        """Seed slot u from user u's training row of the model's own tables.  Rnn and CA-RNN take h from `predict_device` (the rows the
        evaluation path ranks with).  poi_cell_predict does not return the Lstm's cell state, so an Lstm session REPLAYS the users'
        training rows through the session kernels instead: its h then comes from them (float64 state, equal to predict_device's float32
        rows within the test tolerance, not bitwise)."""
        if not self.lstm:
            return super().load_history(users)
        m = self.m
        a = np.arange(m.n_user) if users is None else self._host_ids("users", users, min(m.n_user, self.n_slot))
        if a.size and a.max() >= self.n_slot:
            raise IndexError("users must lie in [0, %d): the session has that many slots" % self.n_slot)
        if len(np.unique(a)) != len(a):
            a = np.unique(a)
        if not a.size:
            return
        off, p = m._off_host.astype(np.int64), m.p.cpu().numpy()
        lens = off[a + 1] - off[a]
        sub = np.concatenate([p[off[u]:off[u + 1]] for u in a]) if lens.sum() else np.zeros(0, np.int64)
        self.reset(a)
        self.replay(np.concatenate(([0], np.cumsum(lens))), sub, slots=a)

    def seed(self, slots, h, last_poi, steps=None, c=None):
        """State from outside (a checkpoint, another model's rows): h (n, dim), last_poi (n) with -1 = none, c (n, dim) for an Lstm
        (zeros when omitted; refused for the other cells)."""
        if c is not None and not self.lstm:
            raise ValueError("only an Lstm session holds a cell state c")
        super().seed(slots, h, last_poi, steps)
        if self.lstm:
            ids = self._slot_tensor(slots)
            if c is None:
                self.c[ids] = 0.0
            else:
                ct = c if isinstance(c, torch.Tensor) else torch.as_tensor(np.asarray(c, np.float64))
                self.c[ids] = ct.to(self.m.device, torch.float64).reshape(ids.numel(), -1)

    def state(self, slots=None):
        """Host copies: dict(h (n, dim) float64, last_poi, steps[, c (n, dim) float64 for an Lstm])."""
        out = super().state(slots)
        if self.lstm:
            out["c"] = np.ascontiguousarray(self.c.index_select(0, self._slot_tensor(slots)).cpu().numpy())
        return out

    # ---- advance --------------------------------------------------------------------------------
    def _launch(self, slot_ptr, poi_ptr, n, hts_out=None, sts_out=None):
        m = self.m
        P = m._cparams(snapshot=True)
        if self.carnn:
            m.ctx.check(m.lib.poi_session_carnn_advance(m.ctx.handle, ctypes.byref(P), _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), m.dd * 1000.0,
                                                        _ptr(self.h), _ptr(self.last_poi), _ptr(self.steps), self.n_slot, ctypes.c_void_p(slot_ptr),
                                                        ctypes.c_void_p(poi_ptr), int(n), _ptr(hts_out), m._stream()))
        else:
            m.ctx.check(m.lib.poi_session_cell_advance(m.ctx.handle, ctypes.byref(P), _ptr(self.h), _ptr(self.c), _ptr(self.last_poi), _ptr(self.steps),
                                                       self.n_slot, ctypes.c_void_p(slot_ptr), ctypes.c_void_p(poi_ptr), int(n), _ptr(hts_out),
                                                       m._stream()))

    # ---- ranking: CA-RNN's own rule ---------------------------------------------------------------
    def _carnn_rows(self, slots):
        """(n, score_rows, has, last POI rows) of the slots: score_rows(o, c) -> poi_carnn_score_all on the CURRENT h and last POI of
        slots o .. o + c - 1, has (n) = the slot has a check-in.  A slot without a check-in has no last POI: it is scored at POI 0 and
        its row masked to -inf, so nothing of it is selectable."""
        m = self.m
        ids = self._slot_tensor(slots)
        users = self.h.index_select(0, ids).float().contiguous()
        lpr = self.last_poi.index_select(0, ids)
        lp, has = lpr.clamp(min=0).contiguous(), lpr >= 0

        def score_rows(o, c):
            full = torch.empty((c, m.n_item), dtype=torch.float32, device=m.device)
            m.ctx.check(m.lib.poi_carnn_score_all(m.ctx.handle, _ptr(users[o:o + c]), _ptr(m.trained_items.t), _ptr(m.M.t), _ptr(m.trained_dists.t),
                                                  _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), _ptr(lp[o:o + c]), c, m.n_item, m.n_dist, m.dim,
                                                  m.dd * 1000.0, _ptr(full), m._stream()))
            return torch.where(has[o:o + c, None], full, torch.full_like(full, float("-inf")))
        return ids.numel(), score_rows, has, lpr

    def _source(self, slots):
        """Lstm / Rnn: Session's fused source (no sts, no distance term).  CA-RNN: its own score rows; what comes out for a slot
        without a check-in is settled by ScoreSource.finish."""
        if not self.carnn:
            return super()._source(slots)
        n, score_rows, has, lpr = self._carnn_rows(slots)
        return ScoreSource(self.m, n, ("last",), lambda: lpr, self._refusals, score_rows=lambda positions=False: score_rows, has=has)

    @staticmethod
    def _refusals():
        """What a call that needs users . items says to a CA-RNN session (ScoreSource.need_fused, _need_fused)."""
        own = "OboCARNN ranks by a score rule of its own"
        dot = own + ", not users . items: "
        return {"near": own + ": within_km / exclude / return_counts are not supported on its sessions",
                "filtered": own + ": within_km is not supported on its sessions",
                "group": dot + "recommend_group is not supported on its sessions (model.recommend_group covers the trained users)",
                "audience": dot + "audience is not supported on its sessions (model.recommend_audience covers the trained users)",
                "route": dot + "recommend_route is not supported on its sessions"}

    def _need_fused(self, family):
        if self.carnn:
            raise _lib.PoiError(self._refusals()[family])


# =================================================================================================
class MfBasic(_Base):
    """public/BPR.py:28-134."""

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, device="cuda:0", init=None, seed=None, table_dtype="f32"):
        """table_dtype="f16": the POI table `lt` and its evaluation snapshot are STORED as IEEE half (float32 arithmetic, snapshot-mode steps only)."""
        self._setup(device, alpha_lambda)
        self.n_user, self.n_item, self.dim = int(n_user), int(n_item), int(n_in)
        self.kdim = self.dim
        if table_dtype not in ("f32", "f16"):
            raise ValueError("table_dtype must be 'f32' or 'f16'")
        self.table_dtype = table_dtype
        self._load_tables(train, test)
        rng = np.random.default_rng(seed) if seed is not None else np.random
        u = lambda *s: rng.uniform(-0.5, 0.5, s)
        init = init or {}
        g = lambda k, v: (init[k] if isinstance(init[k], torch.Tensor) else np.asarray(init[k], np.float64)) if k in init else v()
        tab = (lambda a: self._dev(a).to(torch.float16)) if table_dtype == "f16" else self._dev
        if (n_item + 1) * self.dim > (1 << 28):
            # tables of hundreds of millions of elements (config X: 10 M x 256) are drawn ON the device, as in GruBasic: the host draw is 20 GB of float64
            gen = torch.Generator(device=self.device).manual_seed(0 if seed is None else int(seed))
            u_tab = lambda rows: torch.rand((rows, self.dim), generator=gen, device=self.device, dtype=torch.float32) - 0.5
        else:
            u_tab = lambda rows: u(rows, self.dim)
        self.ux = Shared(self._dev(g("ux", lambda: u(n_user, self.dim))))                  # BPR.py:51
        self.lt = Shared(tab(g("lt", lambda: u_tab(n_item + 1))))                          # :52
        self.trained_items = Shared(tab(u_tab(n_item + 1)))
        self.trained_users = Shared(self._dev(u(n_user, self.dim)))
        if table_dtype == "f16":
            self.ctx.register_f16(self.lt.t); self.ctx.register_f16(self.trained_items.t)

    def __del__(self):
        try:
            if getattr(self, "table_dtype", "f32") == "f16":
                self.ctx.unregister_f16(self.lt.t); self.ctx.unregister_f16(self.trained_items.t)
        except Exception:
            pass

    def update_trained_users(self):
        """public/BPR.py:71-74 (no argument: copies ux)."""
        self.trained_users.t.copy_(self.ux.t)

    # ---- fold-in (poi_foldin_bpr): user rows for check-in histories the model never trained on -----------------------------------------
    # The recurrent models serve an unseen user through a Session slot; this family's only user representation is a trained row, so a
    # new user gets one by running the model's own per-check-in rule on a fresh row against the frozen evaluation snapshot
    # trained_items (width kdim: [lt | fi ei^T] for OboVBpr).  Nothing here changes a parameter or a snapshot.  FPMC-LR and PRME
    # fold in through _SeqFoldin (per-step scalars + the generalised chain), POI2Vec through poi_foldin_p2v (OboPoi2vec.fold_in).  Not covered: the
    # recurrent models (Session).
    def fold_in(self, histories, negatives=None, epochs=10, alpha=None, lam=None, init="zeros", seed=0, return_loss=False, sync=True):
        """User rows for NEW check-in histories (include/poi_hip.h, poi_foldin_bpr): the item side stays frozen and the model's own
        per-check-in SGD rule (public/BPR.py:216-230, :287-306) runs `epochs` times over each history on one fresh row, against the
        evaluation snapshot trained_items.  Returns an (n, kdim) float32 device tensor - rows to rank with exactly like trained_users
        rows ([ux | ue] layout for OboVBpr); with return_loss also the (n, epochs) summed -log sigmoid of every epoch.
        histories: a list of POI id sequences, or a tuple (off, p_flat) CSR of host arrays or device tensors; ids in [0, n_item].
        negatives: None = drawn on the device, once per epoch (poi_sample_negatives on the history CSR: uniform over [0, n_item), redrawn
        while the draw is in the user's own history; epoch e is seeded seed + e - a history must not hold every POI), or an explicit flat
        array of `total` ids (one draw reused by every epoch) or epochs x total ids (epoch-major).
        alpha / lam: default to the model's alpha_lambda[0:2].  init: "zeros", "mean" (the mean row of trained_users) or an (n, kdim) array.
        Host arrays are range-checked before any launch (IndexError).  Device tensors are checked by the kernel: an offending user's row
        and losses are NaN, the other users are untouched, and - with sync - IndexError is raised (sync=False leaves the count to
        ctx.take_bad_ids()).  A user's row does not depend on the other users of the call."""
        off, p, n, total = self._foldin_csr(histories)
        epochs = int(epochs)
        if epochs < 0:
            raise ValueError("epochs must be >= 0 (got %d)" % epochs)
        alpha = self.alpha_lambda[0] if alpha is None else float(alpha)
        lam = self.alpha_lambda[1] if lam is None else float(lam)
        w0 = self._foldin_init(init, n, self.kdim, self.trained_users.t)
        if negatives is None:
            q = torch.empty(max(epochs * total, 1), dtype=torch.int32, device=self.device)
            stride = total
            for e in range(epochs if total else 0):
                self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(off), _ptr(p), n, self.n_item, None, None, 0,
                                                             (int(seed) + e) & 0xFFFFFFFFFFFFFFFF, ctypes.c_void_p(q.data_ptr() + 4 * e * total),
                                                             None, self._stream()))
        else:
            q, stride = self._foldin_given_negatives(negatives, total, epochs)
        w = torch.empty((n, self.kdim), dtype=torch.float32, device=self.device)
        loss = torch.empty((n, epochs), dtype=torch.float32, device=self.device) if return_loss else None
        self.ctx.check(self.lib.poi_foldin_bpr(self.ctx.handle, _ptr(self.trained_items.t), self.n_item, self.kdim, _ptr(off), _ptr(p), _ptr(q), stride,
                                               n, epochs, alpha, lam, _ptr(w0), _ptr(w), _ptr(loss), self._stream()))
        if sync:
            bad = self.ctx.take_bad_ids(self._stream().value)
            if bad:
                raise IndexError("%d history(ies) with an id outside [0, %d] or descending offsets: their rows and losses are NaN" % (bad, self.n_item))
        return (w, loss) if return_loss else w

    def _foldin_rows(self, histories, kw):
        """(folded rows, off, p, n, total) for the ranking entries; the histories are checked with a sync whatever `sync` says - the
        exclusion lists below are built from them."""
        if kw.get("return_loss"):
            raise ValueError("return_loss belongs to fold_in")
        off, p, n, total = csr = self._foldin_csr(histories)
        return (self.fold_in((off, p[:total]), **dict(kw, sync=True)),) + csr

    def recommend_new(self, histories, k, exclude="history", within_km=None, anchor="last", return_scores=False, return_counts=False,
                      sync=True, **fold_in_kwargs):
        """Top-k for NEW users: fold_in(histories, **fold_in_kwargs), then the restricted ranking of compute_sub_topk_near
        (poi_score_topk_near) on the folded rows.  exclude: "history" (each history's distinct POIs leave the candidates), None or a CSR
        pair (off, ids); within_km: only POIs within that many km of the anchor (needs set_coords; None: no radius, no coordinates
        needed); anchor: "last" (each history's last POI; an empty history has none: no radius for it), or one POI id per row (-1: none).
        Returns (n, k) int32 ids, k <= 32, -1 where a row has fewer than k candidates[, scores][, candidate counts]."""
        w, off, p, n, total = self._foldin_rows(histories, fold_in_kwargs)
        if isinstance(anchor, str):
            if anchor != "last":
                raise ValueError("anchor must be 'last' or one POI id per row (got %r)" % (anchor,))
            o = off.long()
            anc = torch.where(o[1:] > o[:-1], p[(o[1:] - 1).clamp(min=0)], torch.full((n,), -1, dtype=torch.int32, device=self.device))
            anc = torch.where(anc >= self.n_item, torch.full_like(anc, -1), anc).contiguous()      # (the padding id has no coordinates)
        else:
            if anchor is None and within_km is not None:
                raise ValueError("within_km needs an anchor: 'last' or one POI id per row")
            anc = self._near_anchor(anchor, n, lambda: None)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        return self._near_launch(w, self.trained_items.t, anc, self._near_radius(within_km), ex, None, k, return_scores, return_counts, sync)

    def rank_new(self, histories, targets, exclude="history", return_scores=False, return_counts=False, sync=True, **fold_in_kwargs):
        """Exact 0-based rank of `targets` ((n, len_t <= 8) POI ids, or a pair (ids, mask)) among all POIs for NEW users:
        fold_in(histories, **fold_in_kwargs), then poi_score_rank on the folded rows, as compute_sub_target_rank.  exclude: "history",
        None or a CSR pair (off, ids); an excluded target is not ranked (-1)."""
        w, off, p, n, total = self._foldin_rows(histories, fold_in_kwargs)
        tgt, tm = self._rank_targets(targets, n)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        return self._rank_launch(w, self.trained_items.t, None, tgt, tm, ex, return_scores, return_counts, sync)


class OboBpr(MfBasic):
    """public/BPR.py:191-241."""

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, **kw):
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, **kw)
        self.params = [self.ux, self.lt]
        self.l2 = _L2(self, ["ux", "lt"])                                                  # :194-197

    def train(self, u_idx, pq_idx):
        """bpr_train(uidx, [p, q]) -> -log sigmoid(u)  (public/BPR.py:234-241)."""
        return float(self.train_batch([u_idx], [pq_idx[0]], [pq_idx[1]])[0])

    def train_batch(self, uidx, p, q, mode="snapshot", sync=True):
        conv = lambda v: v.to(self.device, torch.int32).contiguous() if isinstance(v, torch.Tensor) else \
            torch.as_tensor(np.asarray(v, np.int32)).to(self.device)
        u, pp, qq = conv(uidx), conv(p), conv(q)
        n = u.numel()
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        m = _lib.BPR_HOGWILD if mode == "hogwild" else _lib.BPR_SNAPSHOT
        self.ctx.check(self.lib.poi_bpr_step(self.ctx.handle, _ptr(self.ux.t), _ptr(self.lt.t), self.n_user, self.n_item, self.dim,
                                             _ptr(u), _ptr(pp), _ptr(qq), n, self.alpha_lambda[0], self.alpha_lambda[1],
                                             _ptr(loss), m, self._stream()))
        if sync:
            nb = self.ctx.take_bad_ids(self._stream().value if hasattr(self._stream(), "value") else None)
            if nb:                                     # the reference's gather raises IndexError (public/BPR.py:214-218)
                raise IndexError("%d id(s) outside the user / POI tables in this launch: those triples moved nothing, their losses are NaN" % nb)
        return loss.cpu().numpy() if sync else loss

    def epoch_triples(self):
        """All (user, pos_t, neg_t) triples of the train tables, in the reference's order
        (prog_bpr_gru_spatial.py:240-244) - device int32 tensors."""
        lens = torch.as_tensor(np.diff(self._off_host.astype(np.int64))).to(self.device)
        u = torch.repeat_interleave(self._arange, lens)
        return u, self.p, self.q



class _VbprL2:
    """model.l2 of OboVBpr (public/BPR.py:259-265): 0.5 lambda (|ux|^2 + |lt|^2 + |ue|^2) + 0.5 lambda_ev |ei|^2."""

    def __init__(self, model):
        self.model = model

    def eval(self):
        m = self.model
        out = 0.0
        for names, lam in ((("ux", "lt", "ue"), m.alpha_lambda[1]), (("ei",), m.lambda_ev)):
            acc = torch.zeros(1, dtype=torch.float64, device=m.device)
            for n in names:
                t = getattr(m, n).t
                m.ctx.check(m.lib.poi_sumsq(m.ctx.handle, _ptr(t), t.numel(), _ptr(acc), m._stream()))
            out += 0.5 * lam * float(acc.item())
        return out


class OboVBpr(MfBasic):
    """public/BPR.py:245-335: BPR-MF plus a fixed per-item feature table fi (n_item + 1, n_img) and a trained projection ei (n_in, n_img).
    alpha_lambda = [alpha, lambda, lambda_ev(, fea_random_zero: accepted, unused - the train graph never corrupts features)].
    fea_img: (n_item + 1, n_img) with a zero pad row, or (n_item, n_img) - the pad row is appended.  Float32 tables only."""

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, n_img, fea_img, device="cuda:0", init=None, seed=None):
        if len(alpha_lambda) < 3:
            raise ValueError("OboVBpr: alpha_lambda = [alpha, lambda, lambda_ev(, fea_random_zero)]")
        super().__init__(train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, device=device, init=init, seed=seed)
        self.lambda_ev = float(alpha_lambda[2])
        self.n_img = int(n_img)
        if self.dim % 4 or self.dim > 128 or self.n_img % 4 or not 0 < self.n_img <= 4096:
            raise _lib.PoiError("OboVBpr: n_in must be a multiple of 4 up to 128 and n_img a multiple of 4 up to 4096 (got %d, %d)" % (self.dim, self.n_img))
        fea = fea_img if isinstance(fea_img, torch.Tensor) else np.asarray(fea_img)
        if fea.ndim != 2 or fea.shape[1] != self.n_img or fea.shape[0] not in (self.n_item, self.n_item + 1):
            raise ValueError("fea_img must be (n_item, n_img) or (n_item + 1, n_img); got %s" % (tuple(fea.shape),))
        fi = self._dev(fea)
        if fi.shape[0] == self.n_item:
            fi = torch.cat([fi, torch.zeros((1, self.n_img), dtype=torch.float32, device=self.device)]).contiguous()
        self.fi = Shared(fi)                                                               # BPR.py:249, never trained
        rng = np.random.default_rng(int(seed) + 1) if seed is not None else np.random      # (its own stream: MfBasic drew ux / lt from `seed`)
        u = lambda *s: rng.uniform(-0.5, 0.5, s)
        init = init or {}
        g = lambda k, v: (init[k] if isinstance(init[k], torch.Tensor) else np.asarray(init[k], np.float64)) if k in init else v()
        self.mi = Shared(self._dev(g("mi", lambda: u(self.n_item + 1, self.dim))))         # :252 (set by update_trained_items)
        self.ue = Shared(self._dev(g("ue", lambda: u(self.n_user, self.dim))))             # :253
        self.ei = Shared(self._dev(g("ei", lambda: u(self.dim, self.n_img))))              # :254
        self.kdim = 2 * self.dim
        self.trained_items = Shared(torch.zeros((self.n_item + 1, self.kdim), dtype=torch.float32, device=self.device))
        self.trained_users = Shared(torch.zeros((self.n_user, self.kdim), dtype=torch.float32, device=self.device))
        self.params = [self.ux, self.lt, self.ue, self.ei]                                 # :258
        self.l2 = _VbprL2(self)

    def _vparams(self):
        return _lib.VbprParams(self.ux.t.data_ptr(), self.lt.t.data_ptr(), self.ue.t.data_ptr(), self.ei.t.data_ptr(), self.fi.t.data_ptr(),
                               self.n_user, self.n_item, self.dim, self.n_img)

    def train(self, u_idx, pq_idx):
        """bpr_train(uidx, [p, q]) -> -log sigmoid(x)  (public/BPR.py:312-319)."""
        return float(self.train_batch([u_idx], [pq_idx[0]], [pq_idx[1]])[0])

    def train_batch(self, uidx, p, q, sync=True):
        """One launch of n triples under the batch rule (include/poi_hip.h); n == 1 is the reference step.  sync=True returns the host
        losses and raises IndexError when a triple was rejected (an id outside its table, or p == q: the reference's gather raises on
        the former); sync=False returns the device losses (NaN for rejected triples) and leaves the count to ctx.take_bad_ids()."""
        conv = lambda v: v.to(self.device, torch.int32).contiguous() if isinstance(v, torch.Tensor) else \
            torch.as_tensor(np.asarray(v, np.int32)).to(self.device)
        u, pp, qq = conv(uidx), conv(p), conv(q)
        n = u.numel()
        if pp.numel() != n or qq.numel() != n:
            raise ValueError("uidx, p and q must have the same length")
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        P = self._vparams()
        self.ctx.check(self.lib.poi_vbpr_step(self.ctx.handle, ctypes.byref(P), _ptr(u), _ptr(pp), _ptr(qq), n, self.alpha_lambda[0],
                                              self.alpha_lambda[1], self.lambda_ev, _ptr(loss), self._stream()))
        if sync:
            nb = self.ctx.take_bad_ids(self._stream().value)
            if nb:
                raise IndexError("%d triple(s) with an id outside the user / POI tables or p == q in this launch: they moved nothing, their losses are NaN" % nb)
        return loss.cpu().numpy() if sync else loss

    def epoch_triples(self):
        """All (user, pos_t, neg_t) triples of the train tables in the reference's order - device int32 tensors."""
        lens = torch.as_tensor(np.diff(self._off_host.astype(np.int64))).to(self.device)
        return torch.repeat_interleave(self._arange, lens), self.p, self.q

    def update_trained_items(self):
        """public/BPR.py:321-329: trained_items = [lt | fi ei^T] (the product on the device's matrix cores), mi = its right half."""
        P = self._vparams()
        self.ctx.check(self.lib.poi_vbpr_items(self.ctx.handle, ctypes.byref(P), _ptr(self.trained_items.t), self._stream()))
        self.mi.t.copy_(self.trained_items.t[:, self.dim:])

    def update_trained_users(self):
        """public/BPR.py:331-335: trained_users = [ux | ue]."""
        P = self._vparams()
        self.ctx.check(self.lib.poi_vbpr_users(self.ctx.handle, ctypes.byref(P), _ptr(self.trained_users.t), self._stream()))


# =================================================================================================
class _SeqFoldin:
    """Fold-in of the successive-POI models (include/poi_hip.h, poi_foldin_terms_* / poi_foldin_pair): OboFpmc_lr and OboPrme represent a
    user by one trained row (ui[u], du[u]), so an unseen user gets one by running the model's own per-transition rule on a fresh row with
    the item side frozen.  The terms pass writes each step's scalars a / c off the chain; the chain is poi_foldin_bpr's with them.
    Nothing here changes a model parameter."""

    def _foldin_positions(self, values, total, name, dtype):
        """A per-check-in array of `total` entries -> a flat device tensor (entry 0 of every history is ignored)."""
        if isinstance(values, torch.Tensor) and values.is_cuda:
            t = values.to(self.device).reshape(-1)
            if t.is_floating_point() and dtype == torch.int32 and bool((t != t.round()).any().item()):
                raise ValueError("%s must be whole minutes (the reference's gap is a Theano iscalar)" % name)
            t = t.to(dtype).contiguous()
        else:
            if isinstance(values, (list, tuple)) and len(values) and np.ndim(values[0]) > 0:
                values = np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in values])
            h = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values, np.float64).reshape(-1)
            if dtype == torch.int32:
                if np.any(h != np.round(h)):
                    raise ValueError("%s must be whole minutes (the reference's gap is a Theano iscalar)" % name)
                t = torch.as_tensor(h.astype(np.int64).astype(np.int32)).to(self.device)
            else:
                if not np.all(np.isfinite(h)) or np.any(h < 0):
                    raise ValueError("%s must be finite and >= 0" % name)
                t = torch.as_tensor(h).to(self.device)
        if t.numel() != total:
            raise ValueError("%s must hold one entry per check-in (%d vs %d)" % (name, t.numel(), total))
        return t if total else torch.zeros(1, dtype=dtype, device=self.device)

    def _foldin_seq(self, csr, form, items, mean_of, draw, terms, negatives, epochs, alpha, lam, init, return_loss, sync):
        """The shared body of fold_in: start rows, negatives (draw(e, out) fills epoch e's `total` ids), the terms pass
        (terms(off, p, q, stride, n, total, epochs, c) -> a or None), the chain."""
        off, p, n, total = csr
        epochs = int(epochs)
        if epochs < 0:
            raise ValueError("epochs must be >= 0 (got %d)" % epochs)
        alpha = self.alpha_lambda[0] if alpha is None else float(alpha)
        lam = self.alpha_lambda[1] if lam is None else float(lam)
        w0 = self._foldin_init(init, n, self.dim, mean_of)
        if negatives is None:
            q = torch.empty(max(epochs * total, 1), dtype=torch.int32, device=self.device)
            stride = total
            for e in range(epochs if total else 0):
                draw(e, q[e * total:(e + 1) * total])
        else:
            q, stride = self._foldin_given_negatives(negatives, total, epochs, lo=-1)
        c = torch.empty(max((epochs if stride else 1) * total, 1), dtype=torch.float64, device=self.device)
        a = terms(off, p, q, stride, n, total, epochs, c)
        w = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        loss = torch.empty((n, epochs), dtype=torch.float32, device=self.device) if return_loss else None
        self.ctx.check(self.lib.poi_foldin_pair(self.ctx.handle, _ptr(items), self.n_item, self.dim, form, 1, _ptr(off), _ptr(p), _ptr(q), stride,
                                                _ptr(a), _ptr(c), stride, n, epochs, alpha, lam, _ptr(w0), _ptr(w), _ptr(loss), self._stream()))
        if sync:
            bad = self.ctx.take_bad_ids(self._stream().value)
            if bad:
                raise IndexError("%d history(ies) with an id outside [0, %d] (negatives: -1 skips the step), a bad distance or descending offsets: "
                                 "their rows and losses are NaN" % (bad, self.n_item))
        return (w, loss) if return_loss else w

    def _foldin_last(self, off, p, n):
        """Every history's last POI (n) int32; the ranking entries need one per history (it selects ai[last] / the query POI)."""
        o = off.long()
        if n and not bool((o[1:] > o[:-1]).all().item()):
            raise ValueError("%s ranks a new user from its last check-in: every history needs at least one" % type(self).__name__)
        last = p[(o[1:] - 1).clamp(min=0)].contiguous() if n else torch.zeros(0, dtype=torch.int32, device=self.device)
        if n:
            lo, hi = int(last.min().item()), int(last.max().item())
            if lo < 0 or hi > self.n_item:
                raise IndexError("fold_in histories: ids must lie in [0, %d] (found %d..%d)" % (self.n_item, lo, hi))
        return last

    def _foldin_rows(self, histories, kw, **extra):
        """(folded rows, off, p, n, total, last POIs) for the ranking entries; the histories are checked with a sync whatever `sync`
        says - the exclusion lists are built from them."""
        if kw.get("return_loss"):
            raise ValueError("return_loss belongs to fold_in")
        off, p, n, total = self._foldin_csr(histories)
        last = self._foldin_last(off, p, n)
        w = self.fold_in((off, p[:total]), **dict(kw, sync=True, **extra))
        return w, off, p, n, total, last


class OboFpmc_lr(_SeqFoldin, _Base):
    """public/FPMC_LR.py:27-166 (driver prog_fpmc_lr.py): FPMC with localized regions.  Four tables ui (n_user, D) and iu / ia / ai
    (n_item + 1, D); a transition (u, a = POI at t-1, i = POI at t, j = negative among i's neighbours) moves six rows (poi_fpmc_step).

    train: the reference's [tra_pois, tra_pois_negs, tra_last_poi] (tra_pois_negs is not read: the neighbour sets are built on the device from
    `coords` and `ud_km`, fun_acquire_neighbors_for_each_poi) or a CsrTables (PoiDataset.shard()).  test: [tes_buys_masks, tes_masks,
    tes_buys_neg_masks] (None with CsrTables).  n_size = D (a multiple of 4, <= 128).  Extra keywords: device, init (dict of float64 arrays
    ui / iu / ia / ai), seed, coords ((n_item, 2) lat, lon - required), ud_km (UD, default 20 as prog_fpmc_lr.py:70), max_pairs (refuse neighbour
    sets larger than this)."""

    TABLES = ("ui", "iu", "ia", "ai")

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_size, device="cuda:0", init=None, seed=None, coords=None, ud_km=20.0,
                 max_pairs=1 << 31):
        from .data import ud_threshold
        self.n_user, self.n_item, self.dim = int(n_user), int(n_item), int(n_size)
        if self.dim <= 0 or self.dim % 4 or self.dim > 128:
            raise ValueError("OboFpmc_lr: n_size must be a multiple of 4 in [4, 128] (got %d)" % self.dim)
        if coords is None:
            raise ValueError("OboFpmc_lr needs coords= (the neighbour sets are built on the device from the POI coordinates)")
        off, p, tes = self._host_tables(train, test)
        lens = np.diff(off.astype(np.int64))
        if len(lens) != self.n_user:
            raise ValueError("OboFpmc_lr: %d train sequences for n_user = %d" % (len(lens), self.n_user))
        if np.any(lens <= 0):           # PoiDataset.last_pois() would silently read the previous user's POI
            raise ValueError("OboFpmc_lr: user(s) %s have an empty train sequence (no last POI)" % np.nonzero(lens <= 0)[0][:8].tolist())
        for nm, t in (("train POIs", p), ("test POIs", tes[0]), ("test negatives", tes[2])):
            self._check_ids(nm, t, self.n_item)
        if p.size and p.max() >= self.n_item:
            raise IndexError("train POIs must lie in [0, %d)" % self.n_item)
        self._setup(device, alpha_lambda)
        self.ud_km, self.c_ud = float(ud_km), float(ud_threshold(ud_km))
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        self._off_host, self._lens = off, lens
        self.off, self.p = i32(off), i32(p)
        self.tes_buys_masks, self.tes_masks, self.tes_buys_neg_masks = i32(tes[0]), i32(tes[1]), i32(tes[2])
        self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)
        self.tra_last_poi = i32(p[off[1:].astype(np.int64) - 1])
        xy = np.ascontiguousarray(coords, np.float64)
        if xy.shape != (self.n_item, 2):
            raise ValueError("coords must be (n_item, 2) lat, lon (got %s)" % (xy.shape,))
        self.coords = torch.as_tensor(xy).to(self.device)
        self._cphi = torch.as_tensor(cos_lat(xy)).to(self.device)
        self.nbr_off, self.nbr = self.build_neighbors(max_pairs)
        # transitions t = 1 .. len-1 of every user (prog_fpmc_lr.py:188-190): a target without a neighbour cannot be trained
        # (random.sample(negs[i+1], 1) raises there too)
        cnt = np.diff(self.nbr_off.cpu().numpy())
        first = np.zeros(len(p), bool)
        first[off[:-1].astype(np.int64)] = True
        lonely = np.unique(p[~first][cnt[p[~first]] == 0])
        if lonely.size:
            raise ValueError("OboFpmc_lr: train target POI(s) %s have no neighbour within %g km" % (lonely[:8].tolist(), self.ud_km))
        rng = np.random.default_rng(seed) if seed is not None else np.random
        init = init or {}
        shapes = dict(ui=(self.n_user, self.dim), iu=(self.n_item + 1, self.dim), ia=(self.n_item + 1, self.dim), ai=(self.n_item + 1, self.dim))
        for k in ("ui", "iu", "ia", "ai"):                                                     # FPMC_LR.py:52-59
            v = init[k] if k in init else rng.uniform(-0.5, 0.5, shapes[k])
            t = self._dev(v)
            if tuple(t.shape) != shapes[k]:
                raise ValueError("init[%r] has shape %s, expected %s" % (k, tuple(t.shape), shapes[k]))
            setattr(self, k, Shared(t))
        self.params = [self.ui, self.iu, self.ai, self.ia]                                     # :61
        self.l2 = _L2(self, ["ui", "iu", "ai", "ia"])                                          # :62-64
        self._version, self._items_cat = 0, None

    def _host_tables(self, train, test):
        if isinstance(train, CsrTables):
            off = np.ascontiguousarray(train.off, np.int32)
            return off, np.ascontiguousarray(train.p, np.int32), (np.asarray(train.tes_p), np.asarray(train.tes_mask), np.asarray(train.tes_q))
        tra_pois = train[0]
        lens = np.array([len(s) for s in tra_pois], np.int64)
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        p = np.array([x for s in tra_pois for x in s], np.int64).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
        return off.astype(np.int32), p, tuple(np.asarray(t) for t in test)

    # ---- neighbour sets / negatives -----------------------------------------------------------
    def build_neighbors(self, max_pairs=1 << 31):
        """(off int64 (n_item + 1), ids int32) of neighbours(i) = {k != i : cal_dis(i, k) <= UD} on the device (Load_Data_fpmc_lr.py:114-143):
        a count pass, then - if the total is at most max_pairs - the fill pass into a buffer of exactly that size."""
        order = torch.argsort(self.coords[:, 0], stable=True).to(torch.int32).contiguous()
        off = torch.empty(self.n_item + 1, dtype=torch.int64, device=self.device)
        self.ctx.check(self.lib.poi_fpmc_neighbor_counts(self.ctx.handle, _ptr(self.coords), _ptr(self._cphi), _ptr(order), self.n_item, self.c_ud,
                                                         _ptr(off), self._stream()))
        total = int(off[-1].item())
        if total > max_pairs:
            raise _lib.PoiError("FPMC-LR neighbour sets hold %d pairs (%.1f per POI at UD = %g km), above the limit of %d"
                                % (total, total / self.n_item, self.ud_km, max_pairs))
        nbr = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
        self.ctx.check(self.lib.poi_fpmc_neighbor_fill(self.ctx.handle, _ptr(self.coords), _ptr(self._cphi), _ptr(order), self.n_item, self.c_ud,
                                                       _ptr(off), _ptr(nbr), self._stream()))
        return off, nbr

    def sample_negatives(self, pos, seed):
        """One uniform draw from neighbours(pos[t]) per entry (prog_fpmc_lr.py:190, random.sample(negs[i+1], 1)); device int32."""
        pos = pos.to(self.device, torch.int32).contiguous()
        out = torch.empty_like(pos)
        self.ctx.check(self.lib.poi_fpmc_sample_negatives(self.ctx.handle, _ptr(self.nbr_off), _ptr(self.nbr), self.n_item, _ptr(pos), pos.numel(),
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), self._stream()))
        return out

    def epoch_transitions(self, seed, order=None):
        """All transitions of an epoch in the reference's order (prog_fpmc_lr.py:183-190: users in `order` - default 0..n_user-1 -, positions
        t = 1 .. len-1, a = p[t-1], i = p[t]) with fresh negatives from the device sampler: device int32 tensors (u, a, i, j)."""
        off = self._off_host.astype(np.int64)
        users = np.arange(self.n_user) if order is None else np.asarray(order, np.int64)
        lens = self._lens[users] - 1
        starts = np.repeat(off[users] + 1 - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
        pos = torch.as_tensor(starts + np.arange(int(lens.sum()))).to(self.device)
        u = torch.as_tensor(np.repeat(users, lens).astype(np.int32)).to(self.device)
        i = self.p.index_select(0, pos)
        a = self.p.index_select(0, pos - 1)
        return u, a, i, self.sample_negatives(i, seed)

    def update_neg_masks(self, tes_buys_neg_masks):
        """FPMC_LR.py:71-73: new test negatives every epoch."""
        self._check_ids("test negatives", tes_buys_neg_masks, self.n_item)
        self.tes_buys_neg_masks = self._dev(tes_buys_neg_masks, torch.int32)

    def resample_test_negatives_device(self, seed):
        """fun_random_neg_masks_tes (Load_Data_fpmc_lr.py:81-99) on the device: poi_sample_negatives' test output (the train draw it makes
        alongside goes to a scratch buffer - FPMC-LR's train negatives come from the neighbour sets)."""
        scratch = torch.empty_like(self.p)
        tq = torch.empty_like(self.tes_buys_masks)
        self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(self.off), _ptr(self.p), self.n_user, self.n_item,
                                                     _ptr(self.tes_buys_masks), _ptr(self.tes_masks), self.tes_masks.shape[1],
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(scratch), _ptr(tq), self._stream()))
        self.tes_buys_neg_masks = tq

    # ---- training -----------------------------------------------------------------------------
    def _fparams(self):
        return _lib.FpmcParams(*[ctypes.c_void_p(getattr(self, k).t.data_ptr()) for k in ("ui", "iu", "ia", "ai")], self.n_user, self.n_item, self.dim)

    def train(self, uidx, aidx, iidx, jidxs):
        """seq_train(uidx, aidx, [iidx] + jidxs) (FPMC_LR.py:153-163) with the driver's one negative -> log sigmoid(x)."""
        j = list(np.atleast_1d(np.asarray(jidxs)))
        if len(j) != 1:
            raise ValueError("OboFpmc_lr.train takes one negative per transition (prog_fpmc_lr.py:190); got %d" % len(j))
        return float(self.train_batch([uidx], [aidx], [iidx], j)[0])

    def train_batch(self, u, a, i, j, sync=True):
        """A launch of n transitions (poi_fpmc_step, batch semantics of include/poi_hip.h) -> log sigmoid(x) per transition.  With sync, a
        launch that held a transition with an id outside its table (or i == j) raises IndexError - those transitions moved nothing."""
        conv = lambda v: v.to(self.device, torch.int32).contiguous() if isinstance(v, torch.Tensor) else \
            torch.as_tensor(np.asarray(v, np.int64).astype(np.int32)).to(self.device)
        u, a, i, j = conv(u), conv(a), conv(i), conv(j)
        n = u.numel()
        if not (a.numel() == i.numel() == j.numel() == n):
            raise ValueError("u, a, i, j must have the same length")
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        P = self._fparams()
        self.ctx.check(self.lib.poi_fpmc_step(self.ctx.handle, ctypes.byref(P), _ptr(u), _ptr(a), _ptr(i), _ptr(j), n, self.alpha_lambda[0],
                                              self.alpha_lambda[1], _ptr(loss), self._stream()))
        self._version += 1
        if sync:
            nb = self.ctx.take_bad_ids(self._stream().value)
            if nb:
                raise IndexError("%d transition(s) with an id outside its table or i == j in this launch: they moved nothing, their losses are NaN" % nb)
        return loss.cpu().numpy() if sync else loss

    # ---- evaluation (FPMC_LR.py:75-104): live tables, [ui | ai[last]] . [iu | ia] at width 2 D ----------------------------------------
    @property
    def kdim(self):
        return 2 * self.dim

    def _items(self):
        """(n_item + 1, 2 D) item concatenation, rebuilt once after the tables moved (once per evaluation)."""
        if self._items_cat is None or self._items_cat[0] != self._version:
            self._items_cat = (self._version, torch.cat([self.iu.t, self.ia.t], 1).contiguous())
        return self._items_cat[1]

    def _users_rows(self, start_end):
        ids, lo = self._ids(start_end)
        last = self._rows(self.tra_last_poi, ids, lo)
        return ids, torch.cat([self._rows(self.ui.t, ids, lo), self.ai.t.index_select(0, last.long())], 1).contiguous(), lo

    def compute_sub_all_scores_device(self, start_end):
        """FPMC_LR.py:76-82 -> (n, n_item) device tensor."""
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_score_all(self.ctx.handle, _ptr(users), _ptr(self._items()), n, self.n_item, self.kdim, None, None,
                                              _ptr(out), self._stream()))
        return out

    def compute_sub_topk(self, start_end, k, return_scores=False):
        """Valuate.py:132-146 on the FPMC-LR scores through the fused top-K kernel: (n, k) int32 ids by descending score."""
        if k > 32:
            return self._topk_from_scores(start_end, k, return_scores)
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
        seed = self._seed_begin(lo, n, k)
        self.ctx.check(self.lib.poi_score_topk(self.ctx.handle, _ptr(users), _ptr(self._items()), n, self.n_item, self.kdim, None, None, int(k),
                                               _ptr(idx), _ptr(sc), self._stream()))
        self._seed_end(seed, idx)
        return (idx, sc) if return_scores else idx

    def _last_train_poi(self):
        return self.tra_last_poi

    def compute_sub_topk_near(self, start_end, k, within_km=None, exclude=None, anchor=None, **kw):
        """The restricted-candidate protocol of the FPMC-LR paper: within_km defaults to the model's own UD (ud_km), so that a row's
        candidates are neighbours(last POI) + the last POI itself; within_km=float("inf") lifts the radius."""
        return super().compute_sub_topk_near(start_end, k, self.ud_km if within_km is None else within_km, exclude, anchor, **kw)

    # ---- fold-in: ui rows for check-in histories the model never trained on -------------------------------------------------------------
    def fold_in(self, histories, negatives=None, epochs=10, alpha=None, lam=None, init="zeros", seed=0, return_loss=False, sync=True):
        """Rows of ui for NEW check-in histories (include/poi_hip.h, poi_foldin_terms_fpmc + poi_foldin_pair): iu / ia / ai stay frozen and
        the ui part of the model's own transition rule (public/FPMC_LR.py:113-140) runs `epochs` times over each history's transitions
        t = 1 .. len - 1 on one fresh row.  Returns an (n, D) float32 device tensor[, the (n, epochs) summed -log sigmoid of every epoch].
        histories: a list of POI id sequences or a CSR (off, p_flat), host or device; ids in [0, n_item].  negatives: None = drawn per
        epoch from the targets' neighbour sets (sample_negatives(targets, seed + e); a target without a neighbour gets -1 and its step
        is skipped), or `total` / epochs x total ids at the CSR positions (position 0 of a history is ignored; -1 skips the step).
        alpha / lam: default to alpha_lambda[0:2].  init: "zeros", "mean" (the mean row of ui) or an (n, D) array.  Host data is checked
        before any launch (IndexError); device data by the kernel: an offending history's row and losses are NaN, the others are
        untouched, and - with sync - IndexError is raised (sync=False leaves the count to ctx.take_bad_ids())."""
        csr = self._foldin_csr(histories)
        P = self._fparams()

        def draw(e, out):
            out.copy_(self.sample_negatives(csr[1][:csr[3]], int(seed) + e))

        def terms(off, p, q, stride, n, total, epochs, c):
            self.ctx.check(self.lib.poi_foldin_terms_fpmc(self.ctx.handle, ctypes.byref(P), _ptr(off), _ptr(p), _ptr(q), stride, n, total, epochs,
                                                          _ptr(c), self._stream()))
            return None
        return self._foldin_seq(csr, _lib.FOLDIN_DOT, self.iu.t, self.ui.t, draw, terms, negatives, epochs, alpha, lam, init, return_loss, sync)

    def _foldin_users(self, w, last):
        return torch.cat([w, self.ai.t.index_select(0, last.long())], 1).contiguous()

    def recommend_new(self, histories, k, exclude="history", within_km=None, anchor="last", return_scores=False, return_counts=False,
                      sync=True, **fold_in_kwargs):
        """Top-k for NEW users: fold_in(histories, **fold_in_kwargs), then the rows [w | ai[last POI]] against [iu | ia] through the
        restricted ranking of compute_sub_topk_near.  exclude: "history", None or a CSR pair (off, ids); within_km: only POIs within
        that many km of the anchor (None: no radius; model.ud_km gives the paper's protocol); anchor: "last" (each history's last POI)
        or one POI id per row (-1: none).  Every history needs at least one check-in.  Returns (n, k) int32 ids, k <= 32, -1 where a
        row has fewer than k candidates[, scores][, candidate counts]."""
        w, off, p, n, total, last = self._foldin_rows(histories, fold_in_kwargs)
        if isinstance(anchor, str):
            if anchor != "last":
                raise ValueError("anchor must be 'last' or one POI id per row (got %r)" % (anchor,))
            anc = torch.where(last >= self.n_item, torch.full_like(last, -1), last).contiguous()      # (the padding id has no coordinates)
        else:
            if anchor is None and within_km is not None:
                raise ValueError("within_km needs an anchor: 'last' or one POI id per row")
            anc = self._near_anchor(anchor, n, lambda: None)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        return self._near_launch(self._foldin_users(w, last), self._items(), anc, self._near_radius(within_km), ex, None, k, return_scores,
                                 return_counts, sync)

    def rank_new(self, histories, targets, exclude="history", return_scores=False, return_counts=False, sync=True, **fold_in_kwargs):
        """Exact 0-based rank of `targets` ((n, len_t <= 8) POI ids, or a pair (ids, mask)) among all POIs for NEW users: fold_in, then
        poi_score_rank on the rows [w | ai[last POI]], as compute_sub_target_rank.  exclude: "history", None or a CSR pair."""
        w, off, p, n, total, last = self._foldin_rows(histories, fold_in_kwargs)
        tgt, tm = self._rank_targets(targets, n)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        return self._rank_launch(self._foldin_users(w, last), self._items(), None, tgt, tm, ex, return_scores, return_counts, sync)

    def compute_sub_auc_preference(self, start_end):
        """FPMC_LR.py:84-104 -> bool ndarray (n, len_tes)."""
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        ln = self.tes_masks.shape[1]
        tp, tq, tm = (self._rows(t, ids, lo) for t in (self.tes_buys_masks, self.tes_buys_neg_masks, self.tes_masks))
        out = torch.empty((n, ln), dtype=torch.uint8, device=self.device)
        self.ctx.check(self.lib.poi_auc_preference(self.ctx.handle, _ptr(users), _ptr(self._items()), n, self.kdim, _ptr(tp), _ptr(tq), _ptr(tm),
                                                   ln, _ptr(out), self._stream()))
        return out.cpu().numpy().astype(bool)


# =================================================================================================
class OboPrme(_SeqFoldin, _Base):
    """public/PRME.py:38-219 (driver prog_prme.py): PRME, a pairwise metric embedding with a geographical weight.  Three tables du
    (n_user, D), dp / ds (n_item + 1, D); a transition (u, [p, q, prev], d, gap) moves up to seven rows (poi_prme_step).  Scoring reads the
    `trained_*` snapshots taken by update_trained_items and ranks all POIs by a weighted squared Euclidean distance (poi_prme_score_all /
    poi_prme_score_topk).

    train: the reference's [tra_pois_masks, tra_all_times, tra_all_dists, tra_masks, tra_pois_neg_masks] or a data.PrmeDataset (then test is
    None).  test: [tes_pois_masks, tes_all_times, tes_all_dists, tes_masks, tes_pois_neg_masks] (times / dists are not read).  cordi:
    (n_item + 1, 2) lat, lon with the pad row (`location` of load_data).  n_size = D, a multiple of 4 in [4, 128].  Extra keywords:
    device, init (dict of float64 arrays du / dp / ds), seed."""

    _near_ok = False

    TABLES = ("du", "dp", "ds")

    def __init__(self, train, test, alpha_lambda, threshold, component_weight, cordi, n_user, n_item, n_size, device="cuda:0", init=None,
                 seed=None):
        self.n_user, self.n_item, self.dim = int(n_user), int(n_item), int(n_size)
        if self.dim <= 0 or self.dim % 4 or self.dim > 128:
            raise ValueError("%s: n_size must be a multiple of 4 in [4, 128] (got %d)" % (type(self).__name__, self.dim))
        self.thd, self.cw = int(threshold), float(np.float32(component_weight))
        off, p, dist, gap, q, tes = self._host_tables(train, test)
        lens = np.diff(off.astype(np.int64))
        if len(lens) != self.n_user:
            raise ValueError("%s: %d train sequences for n_user = %d" % (type(self).__name__, len(lens), self.n_user))
        if np.any(lens <= 0):           # the scoring's query POI is the last train POI
            raise ValueError("%s: user(s) %s have an empty train sequence (no last POI)" % (type(self).__name__, np.nonzero(lens <= 0)[0][:8].tolist()))
        for nm, t in (("train POIs", p), ("train negatives", q), ("test POIs", tes[0]), ("test negatives", tes[2])):
            self._check_ids(nm, t, self.n_item)
        if p.max() >= self.n_item:
            raise IndexError("train POIs must lie in [0, %d)" % self.n_item)
        if not np.all(np.isfinite(dist)) or np.any(dist < 0):
            raise ValueError("train distances must be finite and >= 0")
        xy = np.ascontiguousarray(cordi, np.float64)
        if xy.shape != (self.n_item + 1, 2):
            raise ValueError("cordi must be (n_item + 1, 2) lat, lon with the pad row (got %s)" % (xy.shape,))
        self._setup(device, alpha_lambda)
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        self._off_host, self._lens = off, lens
        self.off, self.p, self.q, self.gap = i32(off), i32(p), i32(q), i32(gap)
        self.dist = torch.as_tensor(np.ascontiguousarray(dist, np.float64)).to(self.device)
        self.tes_buys_masks, self.tes_masks, self.tes_buys_neg_masks = i32(tes[0]), i32(tes[1]), i32(tes[2])
        self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)
        self.tra_last_poi = i32(p[off[1:].astype(np.int64) - 1])
        self.cordi = torch.as_tensor(xy).to(self.device)
        rng = np.random.default_rng(seed) if seed is not None else np.random
        init = init or {}
        shapes = dict(ds=(self.n_item + 1, self.dim), dp=(self.n_item + 1, self.dim), du=(self.n_user, self.dim))
        for k in ("ds", "dp", "du"):                                                          # PRME.py:75-78
            v = init[k] if k in init else rng.uniform(-0.5, 0.5, shapes[k])
            t = self._dev(v)
            if tuple(t.shape) != shapes[k]:
                raise ValueError("init[%r] has shape %s, expected %s" % (k, tuple(t.shape), shapes[k]))
            setattr(self, k, Shared(t))
        # trained_* (PRME.py:85-91): scoring reads these snapshots; update_trained_items refreshes them
        self._trained = {k: getattr(self, k).t.clone() for k in self.TABLES}
        self.params = [self.dp, self.ds, self.du]                                             # :163
        self.l2 = _L2(self, ["dp", "ds", "du"])                                               # :165-168

    def _host_tables(self, train, test):
        from .data import PrmeDataset
        if isinstance(train, PrmeDataset):
            ds = train
            q = ds.tra_q if ds.tra_q is not None else np.zeros_like(ds.tra_p)
            tq = ds.tes_q if ds.tes_q is not None else np.full(ds.tes_p.shape, self.n_item, np.int32)
            return (np.asarray(ds.off, np.int32), np.asarray(ds.tra_p, np.int32), np.asarray(ds.tra_d, np.float64), np.asarray(ds.tra_gap, np.int64),
                    np.asarray(q, np.int32), (np.asarray(ds.tes_p), np.asarray(ds.tes_mask), np.asarray(tq)))
        tra_pois, tra_times, tra_dists, tra_masks, tra_neg = (np.asarray(x) for x in train)
        lens = np.asarray(tra_masks, np.int64).sum(axis=1)
        m = np.arange(tra_pois.shape[1])[None, :] < lens[:, None]
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        gap = np.asarray(tra_times, np.float64)[m]
        if np.any(gap != np.round(gap)):
            raise ValueError("check-in time gaps must be whole minutes (the reference's gap is a Theano iscalar)")
        te = [np.asarray(test[0]), np.asarray(test[3]), np.asarray(test[4])]
        return (off.astype(np.int32), tra_pois[m].astype(np.int32), np.asarray(tra_dists, np.float64)[m], gap.astype(np.int64),
                tra_neg[m].astype(np.int32), tuple(te))

    # ---- negatives ----------------------------------------------------------------------------
    def update_neg_masks(self, tra_pois_neg_masks, tes_pois_neg_masks):
        """PRME.py:93-96: new negatives every epoch (padded tables as the reference builds them)."""
        tn = np.asarray(tra_pois_neg_masks)
        m = np.arange(tn.shape[1])[None, :] < self._lens[:, None]
        self._check_ids("train negatives", tn[m], self.n_item)
        self._check_ids("test negatives", tes_pois_neg_masks, self.n_item)
        self.q = self._dev(tn[m], torch.int32)
        self.tes_buys_neg_masks = self._dev(tes_pois_neg_masks, torch.int32)

    def resample_negatives_device(self, seed):
        """fun_random_neg_masks_tra / _tes (Load_Data_prme.py:123-162, prog_prme.py:179-182) on the device: poi_sample_negatives."""
        q = torch.empty_like(self.p)
        tq = torch.empty_like(self.tes_buys_masks)
        self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(self.off), _ptr(self.p), self.n_user, self.n_item,
                                                     _ptr(self.tes_buys_masks), _ptr(self.tes_masks), self.tes_masks.shape[1],
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(q), _ptr(tq), self._stream()))
        self.q, self.tes_buys_neg_masks = q, tq

    def epoch_transitions(self, seed=None, order=None):
        """All transitions of an epoch in the driver's order (prog_prme.py:189-197: users in `order` - default 0..n_user-1 -, positions
        i = 1 .. len-1): device tensors (u, p, q, prev, d, gap) with p = tra[i], q = neg[i], prev = tra[i-1], d = dist[i], gap = gap[i].
        With a seed the negatives are redrawn on the device first (resample_negatives_device)."""
        if seed is not None:
            self.resample_negatives_device(seed)
        off = self._off_host.astype(np.int64)
        users = np.arange(self.n_user) if order is None else np.asarray(order, np.int64)
        lens = self._lens[users] - 1
        starts = np.repeat(off[users] + 1 - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
        pos = torch.as_tensor(starts + np.arange(int(lens.sum()))).to(self.device)
        u = torch.as_tensor(np.repeat(users, lens).astype(np.int32)).to(self.device)
        return (u, self.p.index_select(0, pos), self.q.index_select(0, pos), self.p.index_select(0, pos - 1), self.dist.index_select(0, pos),
                self.gap.index_select(0, pos))

    # ---- training -----------------------------------------------------------------------------
    def _pparams(self, tabs):
        return _lib.PrmeParams(*[ctypes.c_void_p(tabs[k].data_ptr()) for k in ("du", "dp", "ds")], self.n_user, self.n_item, self.dim)

    def train(self, u_idx, pq_idx, ad_idx, t_idx):
        """OboPrme.train(u_idx, [p, q, prev], dist, gap) (PRME.py:216-219) -> log sigmoid(Dq - Dp)."""
        pq = list(np.asarray(pq_idx).reshape(-1))
        if len(pq) != 3:
            raise ValueError("pq_idx must be [p, q, prev] (got %d ids)" % len(pq))
        return float(self.train_batch([u_idx], [pq[0]], [pq[1]], [pq[2]], [ad_idx], [t_idx])[0])

    def train_batch(self, u, p, q, prev, d, gap, sync=True):
        """A launch of n transitions (poi_prme_step, batch semantics of include/poi_hip.h) -> log sigmoid(x) per transition.  With sync, a
        launch that held a rejected transition (an id outside its table, p == q, d not finite or < 0) raises IndexError - those moved
        nothing."""
        conv = lambda v, dt, npdt: v.to(self.device, dt).contiguous() if isinstance(v, torch.Tensor) else \
            torch.as_tensor(np.asarray(v, npdt)).to(dt).to(self.device)
        u, p, q, prev, gap = (conv(v, torch.int32, np.int64) for v in (u, p, q, prev, gap))
        d = conv(d, torch.float64, np.float64)
        n = u.numel()
        if not (p.numel() == q.numel() == prev.numel() == d.numel() == gap.numel() == n):
            raise ValueError("u, p, q, prev, d, gap must have the same length")
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        P = self._pparams({k: getattr(self, k).t for k in self.TABLES})
        self.ctx.check(self.lib.poi_prme_step(self.ctx.handle, ctypes.byref(P), _ptr(u), _ptr(p), _ptr(q), _ptr(prev), _ptr(d), _ptr(gap), n,
                                              self.alpha_lambda[0], self.alpha_lambda[1], self.thd, self.cw, _ptr(loss), self._stream()))
        if sync:
            nb = self.ctx.take_bad_ids(self._stream().value)
            if nb:
                raise IndexError("%d rejected transition(s) in this launch (an id outside its table, p == q, or a bad distance): they moved "
                                 "nothing, their losses are NaN" % nb)
        return loss.cpu().numpy() if sync else loss

    def update_trained_items(self):
        """PRME.py:98-106: the scoring snapshots trained_du / trained_dp / trained_ds <- the live tables."""
        for k in self.TABLES:
            self._trained[k].copy_(getattr(self, k).t)

    # ---- evaluation ---------------------------------------------------------------------------
    def score_rows_device(self, users, qpoi, k=None):
        """Arbitrary (user, query POI) rows against all POIs: (n_rows, n_item) scores, or with k the fused top-K (ids, scores)."""
        users = users.to(self.device, torch.int32).contiguous()
        qpoi = qpoi.to(self.device, torch.int32).contiguous()
        n = users.numel()
        P = self._pparams(self._trained)
        if k is None:
            out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
            self.ctx.check(self.lib.poi_prme_score_all(self.ctx.handle, ctypes.byref(P), _ptr(self.cordi), _ptr(users), _ptr(qpoi), n, self.cw,
                                                       _ptr(out), self._stream()))
            return out
        if not 0 < int(k) <= min(64, self.n_item):
            raise ValueError("k must lie in [1, min(64, n_item)] (got %d)" % int(k))
        idx = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, int(k)), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_prme_score_topk(self.ctx.handle, ctypes.byref(P), _ptr(self.cordi), _ptr(users), _ptr(qpoi), n, self.cw, int(k),
                                                    _ptr(idx), _ptr(sc), self._stream()))
        return idx, sc

    def _query_rows(self, start_end):
        """The reference's rows of one batch (PRME.py:118-120): per user, the last train POI, then the test POIs 0 .. Lb-2 (pad POI beyond
        the user's list), Lb = the batch's longest test list -> (users, qpoi, Lb) device tensors, user-major."""
        ids, lo = self._ids(start_end)
        tm = self._rows(self.tes_masks, ids, lo)
        lb = max(1, int(tm.sum(1).max().item())) if ids.numel() else 1
        tp = self._rows(self.tes_buys_masks, ids, lo)[:, :lb - 1]
        q = torch.cat([self._rows(self.tra_last_poi, ids, lo).view(-1, 1), tp], 1)
        return ids.repeat_interleave(lb), q.reshape(-1).contiguous(), lb

    def compute_sub_all_scores_device(self, start_end):
        """PRME.py:117-139 -> (n * Lb, n_item) device tensor, user-major."""
        users, qpoi, _ = self._query_rows(start_end)
        return self.score_rows_device(users, qpoi)

    def compute_sub_all_scores(self, start_end):
        return self.compute_sub_all_scores_device(start_end).cpu().numpy()

    def compute_sub_topk(self, start_end, k, return_scores=False):
        """Per-user ranking for the metrics: row 0 (query = the last train POI) of each user through the fused top-K -> (n, k) int32 ids.
        (The reference's evaluator zips its n * Lb rows with the n users' test lists; here every user is ranked from its row 0 - see
        INTEGRATION.md.)"""
        ids, lo = self._ids(start_end)
        idx, sc = self.score_rows_device(ids, self._rows(self.tra_last_poi, ids, lo), k)
        return (idx, sc) if return_scores else idx

    _rank_fused = False

    def _diverse_items(self):
        return None                               # two POI tables (preference and sequential space): no single row stands for a POI

    def _rank_score_rows(self, a):
        """The rows compute_sub_topk ranks: every user from its row 0 (query = the last train POI)."""
        ids, lo = self._ids(a)
        return self.score_rows_device(ids, self._rows(self.tra_last_poi, ids, lo)), 1

    # ---- fold-in: du rows for check-in histories the model never trained on -------------------------------------------------------------
    def fold_in(self, histories, gaps, dists=None, negatives=None, epochs=10, alpha=None, lam=None, init="zeros", seed=0, return_loss=False,
                sync=True):
        """Rows of du for NEW check-in histories (include/poi_hip.h, poi_foldin_terms_prme + poi_foldin_pair): the du part of the model's
        own transition rule (public/PRME.py:173-214) runs `epochs` times over each history's transitions t = 1 .. len - 1 on one fresh
        row, against the trained_* snapshots.  Returns an (n, D) float32 device tensor[, the (n, epochs) summed -log sigmoid per epoch -
        the reference's step returns +log sigmoid, fold-in keeps poi_foldin_bpr's sign].
        histories: a list of POI id sequences or a CSR (off, p_flat).  gaps: whole minutes since the previous check-in, one per check-in
        (a flat array or one sequence per history; entry 0 of a history is ignored; fractional gaps raise ValueError as the constructor
        does).  dists: km from the previous check-in, likewise; None = cal_dis of `cordi` on the device.  negatives: None = drawn per
        epoch with poi_sample_negatives on the history CSR (seed + e), or `total` / epochs x total ids at the CSR positions (-1 skips
        the step).  init: "zeros", "mean" (the mean row of the trained du) or an (n, D) array.  Checks and the IndexError-after-sync
        behaviour are OboFpmc_lr.fold_in's; a device distance that is negative or not finite makes a bad history too."""
        csr = self._foldin_csr(histories)
        total = csr[3]
        gap = self._foldin_positions(gaps, total, "gaps", torch.int32)
        dist = None if dists is None else self._foldin_positions(dists, total, "dists", torch.float64)
        P = self._pparams(self._trained)

        def draw(e, out):
            self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(csr[0]), _ptr(csr[1]), csr[2], self.n_item, None, None, 0,
                                                         (int(seed) + e) & 0xFFFFFFFFFFFFFFFF, _ptr(out), None, self._stream()))

        def terms(off, p, q, stride, n, total, epochs, c):
            a = torch.empty(max(total, 1), dtype=torch.float64, device=self.device)
            self.ctx.check(self.lib.poi_foldin_terms_prme(self.ctx.handle, ctypes.byref(P), _ptr(self.cordi), _ptr(off), _ptr(p), _ptr(q), stride,
                                                          _ptr(gap), _ptr(dist), n, total, epochs, self.thd, self.cw, _ptr(a), _ptr(c), self._stream()))
            return a
        return self._foldin_seq(csr, _lib.FOLDIN_METRIC, self._trained["dp"], self._trained["du"], draw, terms, negatives, epochs, alpha, lam, init,
                                return_loss, sync)

    def _foldin_score(self, w, last, o, c, k=None):
        """Rows o .. o + c of the folded table `w` as the du table of a poi_prme_params, query POI = the history's last POI."""
        P = _lib.PrmeParams(ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(self._trained["dp"].data_ptr()), ctypes.c_void_p(self._trained["ds"].data_ptr()),
                            w.shape[0], self.n_item, self.dim)
        users = torch.arange(o, o + c, dtype=torch.int32, device=self.device)
        qp = last[o:o + c].contiguous()
        if k is None:
            out = torch.empty((c, self.n_item), dtype=torch.float32, device=self.device)
            self.ctx.check(self.lib.poi_prme_score_all(self.ctx.handle, ctypes.byref(P), _ptr(self.cordi), _ptr(users), _ptr(qp), c, self.cw, _ptr(out),
                                                       self._stream()))
            return out
        idx = torch.empty((c, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((c, k), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_prme_score_topk(self.ctx.handle, ctypes.byref(P), _ptr(self.cordi), _ptr(users), _ptr(qp), c, self.cw, k, _ptr(idx),
                                                    _ptr(sc), self._stream()))
        return idx, sc

    def _foldin_ex(self, exclude, off, p, n, total):
        """_foldin_exclusion, with the ids of a caller's device lists checked here (no kernel of this path checks them)."""
        eo, ex = self._foldin_exclusion(exclude, off, p, n, total)
        if eo is not None and not isinstance(exclude, str):
            cnt = int(eo[-1].item())
            if eo.numel() != n + 1 or cnt > ex.numel() or bool((eo[1:] < eo[:-1]).any().item()) or int(eo[0].item()) != 0:
                raise ValueError("exclude=(off, ids): off must ascend from 0 to len(ids)")
            if cnt and (int(ex[:cnt].min().item()) < 0 or int(ex[:cnt].max().item()) >= self.n_item):
                raise IndexError("exclude=(off, ids): ids must lie in [0, %d)" % self.n_item)
        return eo, ex

    def recommend_new(self, histories, gaps, k, exclude="history", return_scores=False, return_counts=False, sync=True, **fold_in_kwargs):
        """Top-k for NEW users: fold_in(histories, gaps, **fold_in_kwargs), then the model's own geo-weighted score with the folded rows
        as the du table and each history's last POI as the query POI.  exclude: "history" (each history's distinct POIs leave the
        candidates), None or a CSR pair (off, ids).  Without an exclusion the fused top-K ranks (poi_prme_score_topk); with one, explicit
        score rows - at most 1 GiB at a time - get -inf at the listed ids and go through poi_topk.  k <= min(64, n_item).  Returns (n, k)
        int32 ids by descending score then ascending id, -1 where a row has fewer than k candidates[, scores][, candidate counts]."""
        w, off, p, n, total, last = self._foldin_rows(histories, fold_in_kwargs, gaps=gaps)
        k = int(k)
        if not 0 < k <= min(64, self.n_item):
            raise ValueError("k must lie in [1, min(64, n_item)] (got %d)" % k)
        eo, ex = self._foldin_ex(exclude, off, p, n, total)
        if eo is None:
            idx, sc = self._foldin_score(w, last, 0, n, k) if n else (torch.empty((0, k), dtype=torch.int32, device=self.device),
                                                                        torch.empty((0, k), dtype=torch.float32, device=self.device))
            cnt = torch.full((n,), self.n_item, dtype=torch.int32, device=self.device)
        else:
            eo64 = eo.long()
            row = torch.repeat_interleave(torch.arange(n, device=self.device), eo64[1:] - eo64[:-1])
            ids = ex[:row.numel()].long()

            def score_rows(o, c):
                full = self._foldin_score(w, last, o, c)
                sel = (row >= o) & (row < o + c)
                full[row[sel] - o, ids[sel]] = float("-inf")
                return full
            idx, sc = self._topk_from_rows(score_rows, n, k, True)
            idx = torch.where(sc == float("-inf"), torch.full_like(idx, -1), idx)
            cnt = (self.n_item - (eo64[1:] - eo64[:-1])).int()
        out = (idx,) + ((sc,) if return_scores else ()) + ((cnt,) if return_counts else ())
        return out if len(out) > 1 else idx

    def rank_new(self, histories, gaps=None, targets=None, exclude="history", return_scores=False, return_counts=False, sync=True, **fold_in_kwargs):
        """Exact 0-based rank of `targets` ((n, len_t <= 8) POI ids, or a pair (ids, mask)) among all POIs for NEW users:
        fold_in(histories, gaps, **fold_in_kwargs), explicit score rows (at most 1 GiB at a time) and poi_rank_scores.  exclude:
        "history", None or a CSR pair (off, ids); an excluded target is not ranked (-1)."""
        if gaps is None or targets is None:
            raise ValueError("rank_new needs gaps and targets")
        w, off, p, n, total, last = self._foldin_rows(histories, fold_in_kwargs, gaps=gaps)
        tgt, tm = self._rank_targets(targets, n)
        ex = self._foldin_ex(exclude, off, p, n, total)
        return self._rank_from_scores(lambda o, c: self._foldin_score(w, last, o, c), n, tgt, tm, ex, return_scores, return_counts, sync)

    def compute_sub_auc_preference(self, start_end):
        """PRME.py:141-159 returns zeros (the AUC code is commented out there): AUC is always 0."""
        ids, _ = self._ids(start_end)
        return np.zeros((ids.numel(), self.tes_masks.shape[1]), bool)


class OboPRPRM(OboPrme):
    """public/PRPRM.py: the same model as OboPrme under another class name (prog_prme.py's 'prme' flag 1)."""


# =================================================================================================
class _GeoieL2:
    """model.l2 of GeoIE.py:92-98: 0.5 lambda (|g|^2 + |h|^2 + |t|^2 + |z|^2 + a^2 + b^2)."""

    def __init__(self, model):
        self.model = model

    def eval(self):
        m = self.model
        acc = torch.zeros(1, dtype=torch.float64, device=m.device)
        for n in m.TABLES:
            t = getattr(m, n).t
            m.ctx.check(m.lib.poi_sumsq(m.ctx.handle, _ptr(t), t.numel(), _ptr(acc), m._stream()))
        return 0.5 * m.alpha_lambda[1] * (float(acc.item()) + float((m.ab ** 2).sum().item()))


class OboGeoIE(_Base):
    """public/GeoIE.py:46-194 (driver prog_geoie.py): GeoIE, a pairwise geo-influence model.  Tables g (geo-influence), h (geo-susceptibility),
    z (POI preference) (n_item + 1, D) and t (user preference) (n_user, D); the power law f(d) = a d^b with a, b float64 on the device.  A step of
    one user is a masked all-pairs interaction over the user's whole train sequence (poi_geoie_step); scoring reads the trained_* snapshots
    taken by update_trained.  Two score rules: "reference" - GeoIE.py:117-127, s[u, k] = t[u].z[k] + m_u.h[k]
    (poi_geoie_user_vectors + poi_score_all / poi_score_topk at width 2 D), which drops the power law - and "geo", the rule the step trains:
    s[u, l] = t[u].z[l] + (1 / L) sum_k m_k (g[k].h[l]) f(d(k, l)) over the user's distinct train POIs (poi_geoie_score_all_geo /
    poi_geoie_score_topk_geo).  Under "geo" a user is its history, so unseen histories are served too: score_new / recommend_new / rank_new.

    train: a CsrTables (PoiDataset.shard(); test is then None) or the reference's [tra_buys_masks, tra_buys_neg_masks, tra_count, tra_masks]
    with test = [tes_buys_masks, tes_buys_neg_masks].  coords (n_item, 2) lat, lon - required (the distances are computed on the device).
    n_hidden = D, a multiple of 4 in [4, 128].  Extra keywords: device, init (dict of float64 arrays g / h / t / z and scalars a / b), seed,
    d_min (km; pairs use max(d, d_min), 0 = the reference), score_norm ("reference": the reference's divisor - the sum of the padded id row -,
    "count": the sequence length; INTEGRATION.md - the "reference" rule only), score_rule ("reference" | "geo": the rule of the scoring
    methods when they are called without rule=)."""

    _near_ok = False

    TABLES = ("g", "h", "t", "z")
    RULES = ("reference", "geo")

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_in, n_hidden, coords=None, device="cuda:0", init=None, seed=None,
                 d_min=0.0, score_norm="reference", score_rule="reference"):
        self.n_user, self.n_item, self.dim = int(n_user), int(n_item), int(n_hidden)
        if self.dim <= 0 or self.dim % 4 or self.dim > 128:
            raise ValueError("OboGeoIE: n_hidden must be a multiple of 4 in [4, 128] (got %d)" % self.dim)
        if coords is None:
            raise ValueError("OboGeoIE needs coords= (the pair distances are computed on the device from the POI coordinates)")
        if score_norm not in ("reference", "count"):
            raise ValueError("score_norm must be 'reference' or 'count' (got %r)" % (score_norm,))
        if score_rule not in self.RULES:
            raise ValueError("score_rule must be 'reference' or 'geo' (got %r)" % (score_rule,))
        if not float(d_min) >= 0.0:
            raise ValueError("d_min must be >= 0")
        self.d_min, self.score_norm, self.score_rule = float(d_min), score_norm, score_rule
        off, p, q, tes = self._host_tables(train, test)
        lens = np.diff(off.astype(np.int64))
        if len(lens) != self.n_user:
            raise ValueError("OboGeoIE: %d train sequences for n_user = %d" % (len(lens), self.n_user))
        for nm, t in (("test POIs", tes[0]), ("test negatives", tes[2])):
            self._check_ids(nm, t, self.n_item)
        for nm, t in (("train POIs", p), ("train negatives", q)):
            if t.size and (t.min() < 0 or t.max() >= self.n_item):
                raise IndexError("%s must lie in [0, %d)" % (nm, self.n_item))
        xy = np.ascontiguousarray(coords, np.float64)
        if xy.shape != (self.n_item, 2):
            raise ValueError("coords must be (n_item, 2) lat, lon (got %s)" % (xy.shape,))
        self._setup(device, alpha_lambda)
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        self._off_host, self._lens = off, lens
        self.len_max = int(lens.max()) if len(lens) else 0
        self.off, self.p, self.q = i32(off), i32(p), i32(q)
        self.tes_buys_masks, self.tes_masks, self.tes_buys_neg_masks = i32(tes[0]), i32(tes[1]), i32(tes[2])
        self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)
        self.coords = torch.as_tensor(xy).to(self.device)
        self._cphi = torch.as_tensor(cos_lat(xy)).to(self.device)
        rng = np.random.default_rng(seed) if seed is not None else np.random
        init = init or {}
        shapes = dict(g=(self.n_item + 1, self.dim), h=(self.n_item + 1, self.dim), t=(self.n_user, self.dim), z=(self.n_item + 1, self.dim))
        vals = {}
        for k in ("g", "h", "t", "z", "a", "b"):                                                # GeoIE.py:65-75
            vals[k] = init[k] if k in init else (rng.uniform(-0.5, 0.5, shapes[k]) if k in shapes else rng.uniform(-0.5, 0.5))
        for k in self.TABLES:
            t = self._dev(vals[k])
            if tuple(t.shape) != shapes[k]:
                raise ValueError("init[%r] has shape %s, expected %s" % (k, tuple(t.shape), shapes[k]))
            setattr(self, k, Shared(t))
        self.ab = torch.tensor([float(vals["a"]), float(vals["b"])], dtype=torch.float64, device=self.device)
        self.a, self.b = Shared(self.ab[0:1], scalar=True), Shared(self.ab[1:2], scalar=True)
        self.params = [self.a, self.b]                                                         # :91
        self.l2 = _GeoieL2(self)                                                               # :92-98
        self._trained = {k: getattr(self, k).t.clone() for k in self.TABLES}                  # :81-88 (trained_*)
        self._uvec = self._items_cat = self._geo_train = None
        self.rejected = 0

    def _host_tables(self, train, test):
        if isinstance(train, CsrTables):
            return (np.ascontiguousarray(train.off, np.int32), np.ascontiguousarray(train.p, np.int32), np.ascontiguousarray(train.q, np.int32),
                    (np.asarray(train.tes_p), np.asarray(train.tes_mask), np.asarray(train.tes_q)))
        tra_buys, tra_neg, _, tra_masks = (np.asarray(x) for x in train)
        lens = np.asarray(tra_masks, np.int64).sum(axis=1)
        off, p = padded_to_csr(tra_buys, lens)
        _, q = padded_to_csr(tra_neg, lens)
        tes_p, tes_q = np.asarray(test[0]), np.asarray(test[1])
        return off, p, q, (tes_p, (tes_p < self.n_item).astype(np.int32), tes_q)

    # ---- negatives ----------------------------------------------------------------------------
    def resample_negatives_device(self, seed):
        """fun_random_neg_masks_tra (Load_Data_GeoIE.py:105-121, prog_geoie.py:162-163) - and the test negatives alongside - on the device:
        poi_sample_negatives.  The distances follow on the device inside every step."""
        q = torch.empty_like(self.p)
        tq = torch.empty_like(self.tes_buys_masks)
        self.ctx.check(self.lib.poi_sample_negatives(self.ctx.handle, _ptr(self.off), _ptr(self.p), self.n_user, self.n_item,
                                                     _ptr(self.tes_buys_masks), _ptr(self.tes_masks), self.tes_masks.shape[1],
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(q), _ptr(tq), self._stream()))
        self.q, self.tes_buys_neg_masks = q, tq

    # ---- training -----------------------------------------------------------------------------
    def _gparams(self, tabs):
        return _lib.GeoieParams(*[ctypes.c_void_p(tabs[k].data_ptr()) for k in self.TABLES], ctypes.c_void_p(self.ab.data_ptr()),
                                self.n_user, self.n_item, self.dim)

    def train(self, uidx):
        """GeoIE.train(uidx, dist_pos, dist_neg, msk) (GeoIE.py:190-194): the distances and the mask are built on the device -> loss."""
        return float(self.train_batch([int(uidx)])[0])

    def train_batch(self, uidxs, sync=True):
        """A launch of users (poi_geoie_step, batch semantics of include/poi_hip.h) -> sum_i log sigmoid(sp_i - sq_i) per user.  A rejected user
        (an id out of range, or a non-finite value - d_eff = 0 with b <= 0 included) moved nothing and has a NaN loss; with sync the count is
        added to self.rejected (rejections depend on data and parameters: they are reported, not raised)."""
        a = np.atleast_1d(np.asarray(uidxs.cpu().numpy() if isinstance(uidxs, torch.Tensor) else uidxs)).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_user):
            raise IndexError("user ids must lie in [0, %d) (found %d..%d)" % (self.n_user, int(a.min()), int(a.max())))
        users = torch.as_tensor(a.astype(np.int32)).to(self.device)
        n = int(a.size)
        rows = int(np.maximum(self._lens[a] - 1, 0).sum()) if n else 0
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        P = self._gparams({k: getattr(self, k).t for k in self.TABLES})
        self.ctx.check(self.lib.poi_geoie_step(self.ctx.handle, ctypes.byref(P), _ptr(self.off), _ptr(self.p), _ptr(self.q), _ptr(self.coords),
                                               _ptr(self._cphi), _ptr(users), n, rows, self.alpha_lambda[0], self.alpha_lambda[1], self.d_min,
                                               _ptr(loss), self._stream()))
        if sync:
            self.rejected += self.ctx.take_bad_ids(self._stream().value)
        return loss.cpu().numpy() if sync else loss

    def pair_distances(self, uidxs):
        """poi_geoie_pair_distances of the users: packed float32 (dp, dq) device tensors (data.geoie_pair_distances' order)."""
        a = np.atleast_1d(np.asarray(uidxs)).astype(np.int64)
        rows = np.maximum(self._lens[a] - 1, 0)
        npair = int((rows * (rows + 1) // 2).sum())
        dp = torch.empty(max(npair, 1), dtype=torch.float32, device=self.device)
        dq = torch.empty_like(dp)
        users = torch.as_tensor(a.astype(np.int32)).to(self.device)
        self.ctx.check(self.lib.poi_geoie_pair_distances(self.ctx.handle, _ptr(self.off), _ptr(self.p), _ptr(self.q), self.n_user, self.n_item,
                                                         _ptr(self.coords), _ptr(self._cphi), _ptr(users), len(a), int(rows.sum()), npair,
                                                         _ptr(dp), _ptr(dq), self._stream()))
        return dp[:npair], dq[:npair]

    def update_trained(self):
        """GeoIE.py:104-112: the scoring snapshots trained_g / _h / _t / _z <- the live tables."""
        for k in self.TABLES:
            self._trained[k].copy_(getattr(self, k).t)
        self._uvec = self._items_cat = self._geo_train = None

    # ---- evaluation (GeoIE.py:114-127) --------------------------------------------------------
    @property
    def kdim(self):
        return 2 * self.dim

    def user_vectors(self, norm=None):
        """(n_user, 2 D) [trained_t[u] | m_u] (poi_geoie_user_vectors) for the snapshot; norm defaults to score_norm."""
        norm = self.score_norm if norm is None else norm
        out = torch.empty((self.n_user, 2 * self.dim), dtype=torch.float32, device=self.device)
        P = self._gparams(self._trained)
        self.ctx.check(self.lib.poi_geoie_user_vectors(self.ctx.handle, ctypes.byref(P), _ptr(self.off), _ptr(self.p), self.n_user, self.len_max,
                                                       {"reference": 0, "count": 1}[norm], _ptr(out), self._stream()))
        return out

    def _items(self):
        if self._items_cat is None:
            self._items_cat = torch.cat([self._trained["z"], self._trained["h"]], 1).contiguous()
        return self._items_cat

    def _users_rows(self, start_end):
        if self._uvec is None:
            self._uvec = self.user_vectors()
        ids, lo = self._ids(start_end)
        return ids, self._rows(self._uvec, ids, lo).contiguous(), lo

    def _rule(self, rule):
        rule = self.score_rule if rule is None else rule
        if rule not in self.RULES:
            raise ValueError("rule must be 'reference' or 'geo' (got %r)" % (rule,))
        return rule

    def compute_sub_all_scores(self, start_end, rule=None):
        return self.compute_sub_all_scores_device(start_end, rule).cpu().numpy()

    def compute_sub_all_scores_device(self, start_end, rule=None):
        """(n, n_item) device tensor: GeoIE.py:117-127 under "reference" (the dead ulptai distances are not built), the trained rule on the
        users' train histories and trained_t under "geo"."""
        if self._rule(rule) == "geo":
            ids, lo = self._ids(start_end)
            return self._geo_call(self._geo_train_csr(), ids, self._rows(self._trained["t"], ids, lo).contiguous(), ids.numel())
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
        self.ctx.check(self.lib.poi_score_all(self.ctx.handle, _ptr(users), _ptr(self._items()), n, self.n_item, self.kdim, None, None,
                                              _ptr(out), self._stream()))
        return out

    def compute_sub_topk(self, start_end, k, return_scores=False, rule=None, exclude=None, return_counts=False):
        """Valuate.py:132-146 on the GeoIE scores through the fused top-K kernels: (n, k) int32 ids by descending score.  Under "geo":
        exclude = None, "train" (the user's distinct train POIs leave the candidates) or CSR lists (off, ids) as compute_sub_topk_near
        (k <= 32), -1 / -inf where a row has fewer than k candidates, and with return_counts the candidate count of every row."""
        rule = self._rule(rule)
        if rule != "geo" and (exclude is not None or return_counts):
            raise _lib.PoiError("exclude= / return_counts= belong to the 'geo' rule")
        if k > 32:
            if exclude is not None or return_counts:
                raise _lib.PoiError("exclusion lists and candidate counts need k <= 32 (got %d)" % k)
            return self._topk_from_scores(start_end, k, return_scores, scores=lambda a: self.compute_sub_all_scores_device(a, rule))
        if rule == "geo":
            ids, lo = self._ids(start_end)
            n = ids.numel()
            ex = self._near_exclusion(exclude, n, None, ids, lo, kinds=("train",))
            return self._geo_call(self._geo_train_csr(), ids, self._rows(self._trained["t"], ids, lo).contiguous(), n, int(k), ex, return_scores,
                                  return_counts)
        ids, users, lo = self._users_rows(start_end)
        n = ids.numel()
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
        self.ctx.check(self.lib.poi_score_topk(self.ctx.handle, _ptr(users), _ptr(self._items()), n, self.n_item, self.kdim, None, None, int(k),
                                               _ptr(idx), _ptr(sc), self._stream()))
        return (idx, sc) if return_scores else idx

    # ---- the trained rule (poi_geoie_score_all_geo / poi_geoie_score_topk_geo) ---------------------------------------
    @property
    def _rank_fused(self):
        """Under "geo" the score is not users . items: compute_sub_target_rank goes through explicit score rows + poi_rank_scores."""
        return self.score_rule != "geo"

    def _rank_score_rows(self, a):
        return self.compute_sub_all_scores_device(a), 1

    def _geo_compact(self, off, p, n, total):
        """A history CSR -> the compacted CSR of the scoring entries on the device: (off (n + 1), distinct ascending ids, multiplicities)
        int32, built with torch ops.  The padding id n_item is no check-in and is dropped; any other id outside [0, n_item) is kept as an
        invalid id, so the kernel rejects that row and no other."""
        o = off.long()
        row = torch.repeat_interleave(torch.arange(n, device=self.device), o[1:] - o[:-1])
        ids = p[:total].long()
        ids = torch.where((ids < 0) | (ids > self.n_item), torch.full_like(ids, self.n_item + 1), ids)
        w = self.n_item + 2
        keys, cnt = torch.unique((row * w + ids)[ids != self.n_item], return_counts=True)      # sorted: by row, then by id
        co = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        co[1:] = torch.cumsum(torch.bincount(keys // w, minlength=n), 0)
        pad = lambda t: self._some_ids(t.int().contiguous())
        return co.int(), pad(keys % w), pad(cnt)

    def _geo_train_csr(self):
        """The compacted train histories: built once per snapshot and cached until update_trained."""
        if self._geo_train is None:
            self._geo_train = self._geo_compact(self.off, self.p, self.n_user, int(self._off_host[-1]))
        return self._geo_train

    def _geo_call(self, csr, rows, tu, n, k=None, ex=(None, None), return_scores=False, return_counts=False, sync=True, what="history"):
        """One launch of the trained rule on rows `rows` (None: all) of a compacted CSR with the user rows tu ((n, D) or None = zero):
        the (n, n_item) scores, or idx[, scores][, counts] for k."""
        co, cp, cm = csr
        P = self._gparams(self._trained)
        if k is None:
            out = torch.empty((n, self.n_item), dtype=torch.float32, device=self.device)
            self.ctx.check(self.lib.poi_geoie_score_all_geo(self.ctx.handle, ctypes.byref(P), _ptr(co), _ptr(cp), _ptr(cm), _ptr(tu), _ptr(rows), n,
                                                            _ptr(self.coords), _ptr(self._cphi), self.d_min, _ptr(out), self._stream()))
        else:
            if not 0 < k <= 32:
                raise _lib.PoiError("the fused top-K of the 'geo' rule supports 1 <= k <= 32 (got %d)" % k)
            idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
            sc = torch.empty((n, k), dtype=torch.float32, device=self.device) if return_scores else None
            cnt = torch.empty(n, dtype=torch.int32, device=self.device) if return_counts else None
            self.ctx.check(self.lib.poi_geoie_score_topk_geo(self.ctx.handle, ctypes.byref(P), _ptr(co), _ptr(cp), _ptr(cm), _ptr(tu), _ptr(rows), n,
                                                             _ptr(self.coords), _ptr(self._cphi), self.d_min, _ptr(ex[0]), _ptr(ex[1]), k,
                                                             _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
            out = (idx,) + ((sc,) if return_scores else ()) + ((cnt,) if return_counts else ())
            out = out if len(out) > 1 else idx
        if sync:
            bad = self.ctx.take_bad_ids(self._stream().value)
            if bad:
                raise IndexError("%d %s row(s) with an id outside [0, %d) or a malformed exclusion list: NaN scores / empty lists"
                                 % (bad, what, self.n_item))
        return out

    # ---- unseen users: t never moves in training, so a GeoIE user is its history ------------------------------------------------------------
    def _geo_new(self, histories, user_term):
        off, p, n, total = self._foldin_csr(histories)
        if n and bool((off[1:] < off[:-1]).any().item()):
            raise ValueError("histories=(off, p_flat): off must ascend")
        tu = None
        if user_term is not None:
            tu = self._dev(user_term).reshape(-1, self.dim)
            if tu.shape[0] != n:
                raise ValueError("user_term must hold one row per history (%d vs %d)" % (tu.shape[0], n))
        clean = torch.where((p < 0) | (p > self.n_item), torch.full_like(p, self.n_item), p)      # (the exclusion lists skip invalid ids)
        return self._geo_compact(off, p, n, total), off, clean, n, total, tu

    def score_new(self, histories, user_term=None, sync=True):
        """(n, n_item) device scores of NEW check-in histories (a list of POI id sequences or a CSR (off, p_flat)) under the trained rule
        against the trained_* snapshots: no training, no user id.  user_term: None (tu = 0: an unseen user) or (n, D) rows standing in
        for t[u].  The bits of a history's row do not depend on the other histories of the call.  A device CSR with an id outside
        [0, n_item] gives a NaN row and - with sync - IndexError."""
        csr, off, p, n, total, tu = self._geo_new(histories, user_term)
        return self._geo_call(csr, None, tu, n, sync=sync)

    def recommend_new(self, histories, k, exclude="history", return_scores=False, return_counts=False, user_term=None, sync=True):
        """Top-k (k <= 32) for NEW histories under the trained rule (poi_geoie_score_topk_geo).  exclude: "history" (each history's distinct
        POIs leave the candidates), None or a CSR pair (off, ids).  Returns (n, k) int32 ids by descending score, ties by ascending id,
        -1 where a row has fewer than k candidates[, scores][, candidate counts]."""
        csr, off, p, n, total, tu = self._geo_new(histories, user_term)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        return self._geo_call(csr, None, tu, n, int(k), ex, return_scores, return_counts, sync)

    def rank_new(self, histories, targets, exclude="history", return_scores=False, return_counts=False, sync=True, user_term=None):
        """Exact 0-based rank of `targets` ((n, len_t <= 8) POI ids, or a pair (ids, mask)) among all POIs for NEW histories: score rows
        under the trained rule (at most 1 GiB at a time) + poi_rank_scores.  exclude: "history", None or a CSR pair (off, ids); an
        excluded target is not ranked (-1); a NaN score counts below every target."""
        csr, off, p, n, total, tu = self._geo_new(histories, user_term)
        tgt, tm = self._rank_targets(targets, n)
        ex = self._foldin_exclusion(exclude, off, p, n, total)

        def score_rows(o, c):                            # (with sync a bad history raises here, before its rows are ranked)
            rows = torch.arange(o, o + c, dtype=torch.int32, device=self.device)
            return self._geo_call(csr, rows, tu[o:o + c].contiguous() if tu is not None else None, c, sync=sync)
        return self._rank_from_scores(score_rows, n, tgt, tm, ex, return_scores, return_counts, sync)

    def compute_sub_auc_preference(self, start_end):
        """GeoIE.py:114-115 returns zeros: AUC is always 0."""
        ids, _ = self._ids(start_end)
        return np.zeros((ids.numel(), self.tes_masks.shape[1]), bool)


class OboPoi2vec(_Base):
    """public/POI2Vec.py:36-181 (driver prog_poi2vec.py): POI2Vec.  Tables xu (n_user, D), wl (n_item + 1, D) - the last row is the zero pad
    row wl_m and never moves; .wl exposes the first n_item rows - and pb (n_node, D).  A step of one user is a full softmax over all POIs
    times a hierarchical softmax over the binary region tree (poi_poi2vec_step); scoring reads the trained_* snapshots taken by
    update_trained_params through poi_poi2vec_scores / _topk (the n_node products per row once, not the reference's gather of pb[routes]).

    train / test: a data.Poi2vecDataset as `train` (test is then None), or the reference's five tables [target_masks, context_masks, masks,
    masks_cot, accum_lens] each (Load_Data_Poi2vec.fun_data_masks).  probs / routes / lrs: the (n_item + 1, ..) tables of the tree with the
    pad row; they must come from a perfect binary tree (ValueError otherwise).  n_size = D, a multiple of 4 in [4, 128].  Extra keywords:
    device, init (dict of float64 arrays xu / wl (n_item rows) / pb), seed, softmax_axis ("reference": plu is a softmax over the USERS of
    the evaluation batch, as POI2Vec.py:92 computes it; "items": over the POIs), eval_context ("reference": the contexts of the evaluation
    are read from the TRAIN table at the user's first rows, POI2Vec.py:94-95; "test": the test contexts)."""

    _near_ok = False

    TABLES = ("xu", "wl", "pb")

    def __init__(self, train, test, alpha_lambda, n_user, n_item, n_node, n_size, probs, routes, lrs, device="cuda:0", init=None, seed=None,
                 softmax_axis="reference", eval_context="reference"):
        from .data import Poi2vecDataset
        self.n_user, self.n_item, self.n_node, self.dim = int(n_user), int(n_item), int(n_node), int(n_size)
        if self.dim <= 0 or self.dim % 4 or self.dim > 128:
            raise ValueError("OboPoi2vec: n_size must be a multiple of 4 in [4, 128] (got %d)" % self.dim)
        if softmax_axis not in ("reference", "items"):
            raise ValueError("softmax_axis must be 'reference' or 'items' (got %r)" % (softmax_axis,))
        if eval_context not in ("reference", "test"):
            raise ValueError("eval_context must be 'reference' or 'test' (got %r)" % (eval_context,))
        self.softmax_axis, self.eval_context = softmax_axis, eval_context
        routes, lrs = np.ascontiguousarray(routes, np.int32), np.ascontiguousarray(lrs, np.int8)
        probs = np.ascontiguousarray(probs, np.float32)
        if routes.shape != lrs.shape or routes.ndim != 3 or routes.shape[:2] != (self.n_item + 1, 4) or probs.shape != (self.n_item + 1, 4):
            raise ValueError("routes / lrs must be (n_item + 1, 4, depth) and probs (n_item + 1, 4)")
        self.depth = int(routes.shape[2])
        rid, leaf_nodes = self._route_ids(routes, lrs)
        if isinstance(train, Poi2vecDataset):
            tra = (train.off, train.tra_t, train.tra_coff, train.tra_c)
            tes = (train.tes_off, train.tes_t, train.tes_coff, train.tes_c)
        else:
            tra, tes = self._from_masks(train), self._from_masks(test)
        self._tra = tuple(np.ascontiguousarray(a, np.int32) for a in tra)
        self._tes = tuple(np.ascontiguousarray(a, np.int32) for a in tes)
        self._lens = np.diff(self._tra[0].astype(np.int64))
        if len(self._lens) != self.n_user or len(self._tes[0]) != self.n_user + 1:
            raise ValueError("OboPoi2vec: %d train sequences for n_user = %d" % (len(self._lens), self.n_user))
        for nm, t in (("train targets", self._tra[1]), ("test targets", self._tes[1])):
            if t.size and (t.min() < 0 or t.max() >= self.n_item):
                raise IndexError("%s must lie in [0, %d)" % (nm, self.n_item))
        self.len_max = int(self._lens.max()) if self.n_user else 0
        self._ctx_lens = np.diff(self._tra[2].astype(np.int64))
        self._setup(device, alpha_lambda)
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        self.off, self.tgt, self.coff, self.cidx = (i32(a if a.size else np.zeros(1, np.int32)) for a in self._tra)
        tl = np.diff(self._tes[0].astype(np.int64))
        self.tes_len_max = int(tl.max()) if self.n_user else 0
        msk = np.arange(self.tes_len_max)[None, :] < tl[:, None]
        tes_p = np.full(msk.shape, self.n_item, np.int32)
        tes_p[msk] = self._tes[1]
        self.tes_masks, self.tes_buys_masks = i32(msk.astype(np.int32)), i32(tes_p)          # tes_masks / tes_target_masks
        self._arange = torch.arange(self.n_user, dtype=torch.int32, device=self.device)
        self.routes, self.rid, self.leaf_nodes = i32(routes), i32(rid), i32(leaf_nodes)
        self.lrs = torch.as_tensor(lrs).to(self.device)
        self.probs = torch.as_tensor(probs).to(self.device)
        rng = np.random.default_rng(seed) if seed is not None else np.random
        init = init or {}
        shapes = dict(xu=(self.n_user, self.dim), wl=(self.n_item, self.dim), pb=(self.n_node, self.dim))
        for k in self.TABLES:                                                                  # POI2Vec.py:63-71
            v = np.asarray(init[k], np.float64) if k in init else rng.uniform(-0.5, 0.5, shapes[k])
            if tuple(v.shape) != shapes[k]:
                raise ValueError("init[%r] has shape %s, expected %s" % (k, tuple(v.shape), shapes[k]))
            if k == "wl":
                v = np.concatenate([v, np.zeros((1, self.dim))])                               # wl_m (:67, 134)
            setattr(self, "_" + k, self._dev(v))
        self.xu, self.pb = Shared(self._xu), Shared(self._pb)
        self.wl = Shared(self._wl[:self.n_item])
        self.params = [self.wl]                                                                # :114
        self.l2 = _L2(self, ["xu", "pb", "wl"])                                                # :115-122
        self._trained = {k: getattr(self, "_" + k).clone() for k in self.TABLES}              # :73-79 (trained_users / _items / _branch)
        self.rejected = 0

    def _route_ids(self, routes, lrs):
        """Left-to-right leaf index of every route from its lrs (bit d - 1 = the child taken at route position d), and the node list of
        each leaf; checks that the tables describe one perfect binary tree."""
        dep = self.depth
        if dep < 1 or dep > 31 or self.n_node != (1 << dep) - 1:
            raise ValueError("OboPoi2vec: n_node = %d is not 2^depth - 1 for depth %d (the tree must be perfect)" % (self.n_node, dep))
        if routes.min() < 0 or routes.max() >= self.n_node or not np.all(np.abs(lrs) == 1) or not np.all(lrs[:, :, 0] == 1):
            raise ValueError("OboPoi2vec: routes must lie in [0, n_node) and lrs be +1 / -1 (+1 at the leaf)")
        rid = np.zeros(routes.shape[:2], np.int64)
        for d in range(1, dep):
            rid |= ((1 - lrs[:, :, d].astype(np.int64)) // 2) << (d - 1)
        leaf_nodes = np.full((1 << (dep - 1), dep), -1, np.int64)
        leaf_nodes[rid.reshape(-1)] = routes.reshape(-1, dep)
        if not np.array_equal(leaf_nodes[rid.reshape(-1)], routes.reshape(-1, dep)):
            raise ValueError("OboPoi2vec: two routes with the same turns list different nodes (not one binary tree)")
        leaf_nodes[leaf_nodes < 0] = 0                                                         # leaves no POI reaches: never gathered
        return rid.astype(np.int32), leaf_nodes.astype(np.int32)

    def _from_masks(self, tabs):
        """fun_data_masks' five tables -> CSR of CSR (ids >= n_item are padding)."""
        target_masks, context_masks, masks, masks_cot, accum = (np.asarray(x) for x in tabs)
        lens = np.asarray(masks, np.int64).reshape(len(accum), -1).sum(axis=1)
        off, t = padded_to_csr(np.asarray(target_masks).reshape(len(accum), -1), lens)
        clens = np.asarray(masks_cot, np.int64).sum(axis=1)
        coff, c = padded_to_csr(context_masks, clens)
        return off, t, coff, c

    # ---- training -----------------------------------------------------------------------------
    def _pparams(self, tabs):
        return _lib.Poi2vecParams(*[ctypes.c_void_p(tabs[k].data_ptr()) for k in self.TABLES], _ptr(self.routes), _ptr(self.lrs), _ptr(self.probs),
                                  _ptr(self.rid), self.n_user, self.n_item, self.n_node, self.depth, self.dim)

    def _live(self):
        return {k: getattr(self, "_" + k) for k in self.TABLES}

    def train(self, uidx):
        """Poi2vec.train(uidx) (POI2Vec.py:180-181) -> upq."""
        return float(self.train_batch([int(uidx)])[0])

    def train_batch(self, uidxs, sync=True):
        """A launch of users (poi_poi2vec_step, batch semantics of include/poi_hip.h) -> upq per user.  A rejected user (no train target, a
        non-finite loss) moved nothing and has a NaN loss; with sync the count is added to self.rejected."""
        a = np.atleast_1d(np.asarray(uidxs.cpu().numpy() if isinstance(uidxs, torch.Tensor) else uidxs)).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_user):
            raise IndexError("user ids must lie in [0, %d) (found %d..%d)" % (self.n_user, int(a.min()), int(a.max())))
        return self._launch(a, sync)

    def _launch(self, a, sync=True):
        n = int(a.size)
        ok = a[(a >= 0) & (a < self.n_user)]
        off, coff = self._tra[0].astype(np.int64), self._tra[2].astype(np.int64)
        n_pos = int(self._lens[ok].sum()) if ok.size else 0
        n_ctx = int((coff[off[ok + 1]] - coff[off[ok]]).sum()) if ok.size else 0
        users = torch.as_tensor(a.astype(np.int32)).to(self.device)
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        P = self._pparams(self._live())
        self.ctx.check(self.lib.poi_poi2vec_step(self.ctx.handle, ctypes.byref(P), _ptr(self.off), _ptr(self.tgt), _ptr(self.coff), _ptr(self.cidx),
                                                 _ptr(users), n, n_pos, n_ctx, self.len_max, self.alpha_lambda[0], self.alpha_lambda[1],
                                                 _ptr(loss), self._stream()))
        if sync:
            self.rejected += self.ctx.take_bad_ids(self._stream().value)
        return loss.cpu().numpy() if sync else loss

    def update_trained_params(self):
        """POI2Vec.py:81-89: trained_users / trained_items / trained_branch <- the live tables."""
        for k in self.TABLES:
            self._trained[k].copy_(getattr(self, "_" + k))

    # ---- evaluation (POI2Vec.py:91-112) -------------------------------------------------------
    def _eval_rows(self, a, length=None, eval_context=None):
        """The context rows (CSR on the device) of the evaluation rows (user, t), t < length = the longest test sequence of the batch (:93)."""
        mode = self.eval_context if eval_context is None else eval_context
        tl = np.diff(self._tes[0].astype(np.int64))[a]
        length = int(tl.max()) if length is None and len(a) else int(length or 0)
        src = self._tra if mode == "reference" else self._tes
        off, coff, c = src[0].astype(np.int64), src[2].astype(np.int64), src[3]
        rows = []
        for u in a:
            for t in range(length):
                x = off[u] + t
                if x >= off[u + 1]:
                    if mode == "reference":                                                    # :94-95 would read the next user's rows
                        raise ValueError("eval_context='reference': user %d has %d train positions, the evaluation reads %d" % (u, off[u + 1] - off[u], length))
                    rows.append(c[0:0])
                else:
                    rows.append(c[coff[x]:coff[x + 1]])
        rc = np.zeros(len(rows) + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=rc[1:])
        flat = np.concatenate(rows).astype(np.int32) if len(rows) and rc[-1] else np.zeros(1, np.int32)
        return length, torch.as_tensor(rc).to(self.device), torch.as_tensor(flat).to(self.device)

    def _score_call(self, start_end, k=None, return_scores=False, softmax_axis=None, eval_context=None, length=None):
        a = np.atleast_1d(np.asarray(start_end.cpu().numpy() if isinstance(start_end, torch.Tensor) else start_end)).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.n_user):
            raise IndexError("user ids must lie in [0, %d) (found %d..%d)" % (self.n_user, int(a.min()), int(a.max())))
        axis = {"reference": 0, "items": 1}[self.softmax_axis if softmax_axis is None else softmax_axis]
        length, rc, flat = self._eval_rows(a, length, eval_context)
        users = torch.as_tensor(a.astype(np.int32)).to(self.device)
        rows = len(a) * length
        P = self._pparams(self._trained)
        if k is None:
            out = torch.empty((rows, self.n_item), dtype=torch.float32, device=self.device)
            self.ctx.check(self.lib.poi_poi2vec_scores(self.ctx.handle, ctypes.byref(P), _ptr(self.leaf_nodes), _ptr(users), len(a), length, _ptr(rc),
                                                       _ptr(flat), axis, _ptr(out), self._stream()))
            return out
        idx = torch.empty((rows, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((rows, k), dtype=torch.float32, device=self.device) if return_scores else None
        self.ctx.check(self.lib.poi_poi2vec_topk(self.ctx.handle, ctypes.byref(P), _ptr(self.leaf_nodes), _ptr(users), len(a), length, _ptr(rc),
                                                 _ptr(flat), axis, int(k), _ptr(idx), _ptr(sc), self._stream()))
        return (idx, sc) if return_scores else idx

    def compute_sub_all_scores_device(self, start_end, **kw):
        """POI2Vec.py:91-109 -> (n_batch * length, n_item) device tensor, rows ordered (user, position)."""
        return self._score_call(start_end, **kw)

    def compute_sub_all_scores(self, start_end, **kw):
        return self.compute_sub_all_scores_device(start_end, **kw).cpu().numpy()

    def compute_sub_topk(self, start_end, k, return_scores=False, **kw):
        """Valuate.py:132-146 on the POI2Vec scores: (n_batch * length, k) int32 ids by descending score (ties: ascending id)."""
        if not 1 <= int(k) <= min(64, self.n_item):
            raise _lib.PoiError("top-K supports 1 <= k <= min(64, n_item) (got %d)" % k)
        return self._score_call(start_end, k=int(k), return_scores=return_scores, **kw)

    _rank_fused = False

    def _diverse_items(self):
        return self._trained["wl"]

    def _rank_score_rows(self, a):
        """The rows compute_sub_topk ranks: (user, position) for position < the longest test sequence of the users."""
        full = self._score_call(a)
        return full, (full.shape[0] // max(len(a), 1) if len(a) else 1)

    def _rank_chunk(self, n):
        if self.softmax_axis == "reference":
            return max(n, 1)                      # the reference softmax runs over the USERS of a call: the call is not cut
        return super()._rank_chunk(n)             # softmax over the POIs: a row does not depend on the other users of its call

    # ---- unseen users (poi_foldin_p2v) ---------------------------------------------------------------------------------
    # paths_i of Poi2vec.seq_train (POI2Vec.py:140-163) depends on wl, pb and the contexts, never on xu: with the item side frozen the
    # row of a new user sees the full softmax over the POIs alone, and one pass over its history is one gradient step of
    #   logsumexp_j (w . wl_j) - (1/L) sum_i w . wl_{t_i} + (lambda / 2) |w|^2.
    def fold_in(self, histories, epochs=10, alpha=None, lam=None, init="zeros", seed=0, return_loss=False, sync=True):
        """User rows for NEW check-in histories (include/poi_hip.h, poi_foldin_p2v): the xu[u] part of the reference step
        (POI2Vec.py:140-163) runs `epochs` times - one step per pass over the history - on one fresh row against the evaluation snapshot
        of wl (update_trained_params).  Returns an (n, D) float32 device tensor - rows to score with exactly like trained xu rows; with
        return_loss also the (n, epochs) losses logsumexp - mean target logit, each at the values before its epoch's update.  Changes no
        parameter and no snapshot.
        histories: a list of POI id sequences, or a tuple (off, p_flat) CSR of host arrays or device tensors; ids in [0, n_item) - the
        padding id n_item is not a POI of the softmax and is refused.  alpha / lam: default to the model's alpha_lambda[0:2].
        init: "zeros", "uniform" (the reference's uniform(-0.5, 0.5) rows, POI2Vec.py:63, drawn from `seed`) or an (n, D) array.
        Host arrays are range-checked before any launch (IndexError).  Device tensors are checked by the kernel: an offending history's
        row and losses are NaN, the others are untouched, and - with sync - IndexError is raised (sync=False leaves the count to
        ctx.take_bad_ids()).  A history's row does not depend on the other histories of the call."""
        off, p, n, total = self._foldin_csr(histories)
        on_device = isinstance(histories, tuple) and len(histories) == 2 and isinstance(histories[1], torch.Tensor) and histories[1].is_cuda
        if total and not on_device and int(p[:total].max()) >= self.n_item:
            raise IndexError("fold_in histories: ids must lie in [0, %d) (the padding id is no POI of the softmax)" % self.n_item)
        epochs = int(epochs)
        if epochs < 0:
            raise ValueError("epochs must be >= 0 (got %d)" % epochs)
        alpha = self.alpha_lambda[0] if alpha is None else float(alpha)
        lam = self.alpha_lambda[1] if lam is None else float(lam)
        if isinstance(init, str):
            if init not in ("zeros", "uniform"):
                raise ValueError("init must be 'zeros', 'uniform' or an (n, D) array (got %r)" % (init,))
            w0 = None if init == "zeros" else self._dev(np.random.default_rng(seed).uniform(-0.5, 0.5, (n, self.dim)))
        else:
            w0 = self._foldin_init(init, n, self.dim, None)
        w = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        loss = torch.empty((n, epochs), dtype=torch.float32, device=self.device) if return_loss else None
        self.ctx.check(self.lib.poi_foldin_p2v(self.ctx.handle, _ptr(self._trained["wl"]), self.n_item, self.dim, _ptr(off), _ptr(p), n, epochs,
                                               alpha, lam, _ptr(w0), _ptr(w), _ptr(loss), self._stream()))
        if sync:
            bad = self.ctx.take_bad_ids(self._stream().value)
            if bad:
                raise IndexError("%d history(ies) with an id outside [0, %d) or descending offsets: their rows and losses are NaN" % (bad, self.n_item))
        return (w, loss) if return_loss else w

    def _new_contexts(self, contexts, off, p, n):
        """contexts -> the context CSR (rc (n + 1), flat) int32 on the device, one row per history: "last" (the history's last check-in),
        "none" (empty rows: ind = 0, S = 0, paths = 1 - the score is plu alone) or a list of n id arrays."""
        if isinstance(contexts, str):
            if contexts not in ("last", "none"):
                raise ValueError("contexts must be 'last', 'none' or one id array per history (got %r)" % (contexts,))
            o = off.long()
            has = (o[1:] > o[:-1]) if contexts == "last" else torch.zeros(n, dtype=torch.bool, device=self.device)
            rc = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            rc[1:] = torch.cumsum(has.long(), 0)
            flat = p[(o[1:] - 1).clamp(min=0)][has]
            pad = self._some_ids(flat.int().contiguous())
            return rc.int(), pad
        rows = [np.asarray(c, np.int64).reshape(-1) for c in contexts]
        if len(rows) != n:
            raise ValueError("contexts must hold one id array per history (%d vs %d)" % (len(rows), n))
        flat = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        self._check_ids("contexts", flat, self.n_item)
        rc = np.zeros(n + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=rc[1:])
        i32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
        return i32(rc), i32(flat if flat.size else [0])

    def _foldin_rows(self, histories, contexts, kw):
        """(folded rows, context CSR, off, p, n, total); the histories are checked with a sync whatever `sync` says - the exclusion
        lists and the default contexts are built from them."""
        if kw.get("return_loss"):
            raise ValueError("return_loss belongs to fold_in")
        off, p, n, total = csr = self._foldin_csr(histories)
        return (self.fold_in((off, p[:total]), **dict(kw, sync=True)), self._new_contexts(contexts, off, p, n)) + csr

    def _new_params(self, w):
        tabs = dict(self._trained, xu=w)
        return _lib.Poi2vecParams(*[ctypes.c_void_p(tabs[k].data_ptr()) for k in self.TABLES], _ptr(self.routes), _ptr(self.lrs), _ptr(self.probs),
                                  _ptr(self.rid), max(int(w.shape[0]), 1), self.n_item, self.n_node, self.depth, self.dim)

    def _score_rows_new(self, w, rc, flat, o=0, c=None):
        """poi_poi2vec_scores on rows o .. o + c of the folded rows: n_user = c, users = arange(c), length 1, softmax over the POIs."""
        c = w.shape[0] - o if c is None else c
        out = torch.empty((c, self.n_item), dtype=torch.float32, device=self.device)
        if c:
            wc = w[o:o + c].contiguous()
            rcc = (rc[o:o + c + 1] - rc[o]).contiguous()
            fl = flat[int(rc[o]):] if o else flat
            fl = self._some_ids(fl)
            users = torch.arange(c, dtype=torch.int32, device=self.device)
            P = self._new_params(wc)
            self.ctx.check(self.lib.poi_poi2vec_scores(self.ctx.handle, ctypes.byref(P), _ptr(self.leaf_nodes), _ptr(users), c, 1, _ptr(rcc),
                                                       _ptr(fl.contiguous()), 1, _ptr(out), self._stream()))
        return out

    def score_new(self, histories, contexts="last", **fold_in_kwargs):
        """(n, n_item) device scores paths_j plu_j of NEW histories: fold_in(histories, **fold_in_kwargs), then poi_poi2vec_scores with
        the folded rows in the place of xu (one row per history, length 1).  plu is the softmax over the POIs, always: the reference's
        softmax over the USERS of an evaluation batch (softmax_axis="reference") ties a row's scores to whoever shares its batch, which
        is meaningless between unrelated new users.  contexts: "last" (each history's last check-in), "none" (an empty context: ind = 0,
        S = 0, paths = 1 - the score is plu alone) or one id array per history (data.poi2vec_next_context builds one from timestamps)."""
        w, (rc, flat), off, p, n, total = self._foldin_rows(histories, contexts, fold_in_kwargs)
        return self._score_rows_new(w, rc, flat)

    def recommend_new(self, histories, k, contexts="last", exclude="history", return_scores=False, return_counts=False, within_km=None,
                      sync=True, **fold_in_kwargs):
        """Top-k (k <= min(64, n_item)) for NEW histories: fold_in, then poi_poi2vec_topk_ex on the folded rows (score_new's scores, never
        stored).  exclude: "history" (each history's distinct POIs leave the candidates), None or a CSR pair (off, ids) of ascending
        unique ids per row.  Returns (n, k) int32 ids by descending score, ties by ascending id, -1 (score NaN) where a row has fewer
        than k candidates[, scores][, candidate counts].  within_km is refused: POI2Vec has no restricted ranking."""
        if within_km is not None:
            raise _lib.PoiError("%s ranks by a score rule of its own, not users . items: compute_sub_topk_near does not cover it" % type(self).__name__)
        if not 1 <= int(k) <= min(64, self.n_item):
            raise _lib.PoiError("top-K supports 1 <= k <= min(64, n_item) (got %d)" % k)
        w, (rc, flat), off, p, n, total = self._foldin_rows(histories, contexts, fold_in_kwargs)
        eo, ex = self._foldin_exclusion(exclude, off, p, n, total)
        idx = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, int(k)), dtype=torch.float32, device=self.device) if return_scores else None
        cnt = torch.empty(n, dtype=torch.int32, device=self.device) if return_counts else None
        if n:
            users = torch.arange(n, dtype=torch.int32, device=self.device)
            P = self._new_params(w)
            self.ctx.check(self.lib.poi_poi2vec_topk_ex(self.ctx.handle, ctypes.byref(P), _ptr(self.leaf_nodes), _ptr(users), n, 1, _ptr(rc),
                                                        _ptr(flat), 1, _ptr(eo), _ptr(ex), int(k), _ptr(idx), _ptr(sc), _ptr(cnt), self._stream()))
        if sync:
            torch.cuda.current_stream(self.device).synchronize()
        out = (idx,) + ((sc,) if return_scores else ()) + ((cnt,) if return_counts else ())
        return out if len(out) > 1 else idx

    def rank_new(self, histories, targets, contexts="last", exclude="history", return_scores=False, return_counts=False, within_km=None,
                 sync=True, **fold_in_kwargs):
        """Exact 0-based rank of `targets` ((n, len_t <= 8) POI ids, or a pair (ids, mask)) among all POIs for NEW histories: score_new's
        rows (at most 1 GiB at a time) + poi_rank_scores.  exclude: "history", None or a CSR pair (off, ids); an excluded target is not
        ranked (-1); a NaN score counts below every target."""
        if within_km is not None:
            raise _lib.PoiError("%s ranks by a score rule of its own, not users . items: compute_sub_topk_near does not cover it" % type(self).__name__)
        w, (rc, flat), off, p, n, total = self._foldin_rows(histories, contexts, fold_in_kwargs)
        tgt, tm = self._rank_targets(targets, n)
        ex = self._foldin_exclusion(exclude, off, p, n, total)
        # (the folded rows are scored with the softmax over the POIs whatever softmax_axis says: they are cut like any other model's)
        return self._rank_from_scores(lambda o, c: self._score_rows_new(w, rc, flat, o, c), n, tgt, tm, ex, return_scores, return_counts, sync,
                                      step=_Base._rank_chunk(self, max(n, 1)))

    def compute_sub_auc_preference(self, start_end):
        """POI2Vec.py:111-112 returns zeros: AUC is always 0."""
        ids, _ = self._ids(start_end)
        return np.zeros((ids.numel(), self.tes_masks.shape[1]), bool)
