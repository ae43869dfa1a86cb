"""Epoch loop in the shape of prog_bpr_gru_spatial.py:182-334 (train_valid_or_test) on a PoiDataset:
per-epoch negative refresh -> shuffled user order -> train (one user per step like the reference, or
`batch_users` per launch) -> snapshots -> predict -> evaluate.  The reference's three-way timing split
(train / user vectors / test, :232,264,299,305-310) is kept."""
from __future__ import annotations

import os
import pickle
import time

import numpy as np
import torch

from . import models
from .evaluate import GlobalBest, fun_predict_auc_recall_map_ndcg


def compute_start_end(user_num, size):
    """Params.compute_start_end (prog_bpr_gru_spatial.py:156-179): contiguous np.arange batches."""
    return [np.arange(s, min(s + size, user_num), dtype=np.int32) for s in range(0, user_num, size)]


def default_params():
    """The in-source config of prog_bpr_gru_spatial.py:54-78 (flag 2 = Distance2Pre)."""
    return dict(at_nums=[5, 10, 15, 20], epochs=3, latent_size=20, alpha=0.01, **{"lambda": 0.001}, gru=2,
                batch_size_test=32, batch_users=1, seed=123,
                dataset="synthetic", UD=40, dd=200, load_epoch=0, save_per_epoch=0)       # :54-78 (checkpoint naming / cadence)


def load_dataset(p, root="."):
    """Params.__init__ of the driver (prog_bpr_gru_spatial.py:81-91): p['dataset'] names a sequence file in the ETL's format
    ('Foursquare.txt' / 'Gowalla.txt' under `root`, or any path) -> data.load_sequence_file with p['split'] (-1 test / -2 valid), p['dd'] and
    dist_num = int(UD * 1000 / dd) (:81).  'synthetic' / 'synthetic:<shape>' -> the generator (data.SHAPES)."""
    from . import data as pdata
    name = str(p.get("dataset", "synthetic"))
    dist_num = int(p["UD"] * 1000 / p["dd"])
    if name.startswith("synthetic"):
        shape = name.split(":", 1)[1] if ":" in name else "tiny"
        n_item, n_user, max_len, _ = pdata.SHAPES[shape]
        return pdata.make_synthetic(n_user, n_item, max_len, seed=p.get("seed", 0), dd=p["dd"], ud_km=p["UD"], local=p.get("local", 0.8))
    path = name if os.path.exists(name) else os.path.join(root, name)
    if not os.path.exists(path):
        raise FileNotFoundError("dataset %r: no such sequence file (looked at %s)" % (name, path))
    return pdata.load_sequence_file(path, split=p.get("split", -1), dd=p["dd"], dist_num=dist_num, seed=p.get("seed", 0))


def build_model(ds, p, device="cuda:0", seed=None):
    tab = ds.shard()
    size = p["latent_size"]
    al = [p["alpha"], p["lambda"]]
    if p["gru"] == 0:
        return models.OboBpr(train=tab, test=None, alpha_lambda=al, n_user=ds.n_user, n_item=ds.n_item, n_in=size, n_hidden=size,
                             device=device, seed=seed)
    if p["gru"] == 1:
        return models.OboGru(train=tab, test=None, alpha_lambda=al, n_user=ds.n_user, n_item=ds.n_item, n_in=size, n_hidden=size,
                             device=device, seed=seed)
    if p["gru"] == 3:                                                   # prog_bpr_gru_spatial.py:141-151
        return models.OboCARNN(train=tab, test=None, dist=None, alpha_lambda=al, n_user=ds.n_user, n_item=ds.n_item,
                               n_dists=[ds.dist_num, ds.dd / 1000.0], n_in=size, n_hidden=size, device=device, seed=seed, coords=ds.coords)
    return models.OboSpatialGru(train=tab, test=None, dist=None, alpha_lambda=al, n_user=ds.n_user, n_item=ds.n_item,
                                n_dists=[ds.dist_num, ds.dd / 1000.0], n_in=size, n_hidden=size, device=device, seed=seed,
                                coords=ds.coords)


CKPT_ORDER = ("loss_weight", "wd", "lt", "di", "ui", "wh", "bi", "vs", "bs")      # prog_bpr_gru_spatial.py:325-327


def checkpoint_path(p, model_name, epoch, root="./model"):
    """File name of prog_bpr_gru_spatial.py:207-209,321-322."""
    return os.path.join(root, os.path.basename(str(p["dataset"])), "%s_size%s_UD%s_dd%s_epoch%s" % (model_name, p["latent_size"], p["UD"], p["dd"], epoch))


def _py2_compatible(stream):
    """Rewrite the GLOBAL opcodes of a protocol-2 pickle so that numpy >= 2's private module path
    (numpy._core.multiarray) becomes the public one every numpy since 1.x exports (numpy.core.multiarray): the
    reference unpickles these files with Python 2 + an old numpy, which has no numpy._core.  GLOBAL arguments are
    newline-terminated text ("c<module>\\n<name>\\n"), so the opcode is rewritten in place, opcode by opcode
    (pickletools.genops), never by a blind byte replace that could hit array payload."""
    import pickletools
    ops = list(pickletools.genops(stream))
    out, prev = bytearray(), 0
    for i, (op, arg, pos) in enumerate(ops):
        if op.name == "GLOBAL" and arg.startswith("numpy._core."):
            end = ops[i + 1][2] if i + 1 < len(ops) else len(stream)
            mod, name = arg.split(" ")
            out += stream[prev:pos] + b"c" + mod.replace("numpy._core.", "numpy.core.").encode() + b"\n" + name.encode() + b"\n"
            prev = end
    out += stream[prev:]
    return bytes(out)


def dump_checkpoint(values, path):
    """The reference's checkpoint file (prog_bpr_gru_spatial.py:323-330): a pickled list of the nine parameter
    arrays [loss_weight, wd, lt, di, ui, wh, bi, vs, bs] as float64 (Theano's floatX there), protocol 2 =
    cPickle.HIGHEST_PROTOCOL of Python 2, with module paths an old numpy can import (_py2_compatible) - readable
    by the reference's cPickle.load and by load_checkpoint."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(_py2_compatible(pickle.dumps([np.asarray(v, np.float64) for v in values], protocol=2)))


def read_checkpoint(path):
    """List of nine arrays from a checkpoint written by dump_checkpoint or by the reference (Python 2 pickle)."""
    with open(path, "rb") as f:
        objs = pickle.load(f, encoding="latin1")
    if len(objs) != len(CKPT_ORDER):
        raise ValueError("checkpoint %s holds %d objects, expected %d" % (path, len(objs), len(CKPT_ORDER)))
    return [np.asarray(o) for o in objs]


def save_checkpoint(model, path):
    dump_checkpoint([getattr(model, k).get_value() for k in CKPT_ORDER], path)


def load_checkpoint(model, path):
    """model.load_params(cPickle.load(f)) of prog_bpr_gru_spatial.py:210-213."""
    model.load_params(read_checkpoint(path))


def evaluate_epoch(p, model, best, epoch, starts_ends_auc, starts_ends_tes, tes_buys_masks, tes_masks, full_rank=False):
    """The epoch's evaluation of every driver: fun_predict_auc_recall_map_ndcg, plus - with full_rank=True (p["full_rank"]; off by
    default) - the exact-rank metrics of evaluate.full_rank_metrics (mrr, mean / median rank, auc_full, recall at p["full_rank_at"],
    default [20, 100, 1000] clipped to n_item) under the key "full_rank", which the epoch record then carries."""
    m = fun_predict_auc_recall_map_ndcg(p, model, best, epoch, starts_ends_auc, starts_ends_tes, tes_buys_masks, tes_masks)
    if full_rank:
        from .evaluate import full_rank_metrics
        at = sorted(set(min(int(k), model.n_item) for k in p.get("full_rank_at", [20, 100, 1000])))
        m["full_rank"] = full_rank_metrics(model, starts_ends_tes, at)
    return m


def _full_rank(m):
    return {"full_rank": m["full_rank"]} if "full_rank" in m else {}


def train_valid_or_test(ds, p, device="cuda:0", log=print):
    if ds is None or isinstance(ds, str):                          # a sequence file: BASELINE.json configs[0] through the product
        if isinstance(ds, str):
            p = dict(p, dataset=ds)
        ds = load_dataset(p)
    model = build_model(ds, p, device, seed=p.get("seed"))
    ini_epoch = 0
    if p["gru"] == 2 and p.get("load_epoch", 0):                  # prog_bpr_gru_spatial.py:204-214
        load_checkpoint(model, checkpoint_path(p, model.__class__.__name__, p["load_epoch"], p.get("model_root", "./model")))
        ini_epoch = p["load_epoch"] + 1
    best = GlobalBest(p["at_nums"])
    U = ds.n_user
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    # the reference predicts in batch_size_test-user calls (32 by default: 1563 launches of 0.2 ms per Gowalla epoch = 0.32 s, 30x the
    # training time); the result rows are the same for any chunking, so the predict passes use chunks of >= 16384 users
    ses_pred = compute_start_end(U, max(int(p["batch_size_test"]), 16384))
    tes_p, tes_m = ds.tes_p.reshape(-1, 1), np.ones((U, 1), np.int32)
    lens = ds.lens
    history = []
    rng_neg = np.random.default_rng(p.get("seed", 0) + 1000)
    B = int(p.get("batch_users", 1))
    for epoch in range(ini_epoch, p["epochs"]):
        if epoch > 0:                                               # :221-228 (every epoch after the first, also after a resume)
            if p.get("device_negatives", True):                     # on the GPU: ~0.1 ms instead of ~0.4 s of numpy
                model.resample_negatives_device(p.get("seed", 0) * 1000003 + epoch)
            else:
                ds.resample_negatives(rng_neg)
                model.set_negatives_csr(ds.tra_q, ds.tes_q, ds.tra_dq if p["gru"] in (2, 3) else None)
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U).astype(np.int32)      # :236-238
        loss = 0.0
        if p["gru"] == 0:                                           # :240-244 - one triple per valid position
            u, pp, qq = model.epoch_triples()
            if B <= 1:
                off = ds.off.astype(np.int64)
                hp, hq = model.p.cpu().numpy(), model.q.cpu().numpy()      # current (possibly device-refreshed) tables
                for uidx in order:
                    for i in range(off[uidx], off[uidx + 1]):
                        loss += model.train(int(uidx), [int(hp[i]), int(hq[i])])
            else:
                loss = float(model.train_batch(u, pp, qq, mode="snapshot").sum())
        elif B <= 1 and p["gru"] == 2:                              # :246-254, one launch per user without a host round trip per step
            loss += float(model.train_sequence(order)[:, 0].sum())
        elif B <= 1:
            for uidx in order:
                loss += model.train(np.int32(uidx))
        else:
            # launches of equal size (about B users each): no tiny trailing launch
            Be = -(-U // max(1, int(round(U / float(B)))))
            for b0 in range(0, U, Be):
                ids = order[b0:b0 + Be]
                ids = ids[np.argsort(-lens[ids], kind="stable")]
                out = model.train_batch(ids)
                loss += float(out[:, 0].sum()) if p["gru"] == 2 else float(out.sum())
        l2 = model.l2.eval()                                        # :255
        t1 = time.time()
        model.update_trained_items()                                # :266-298
        if p["gru"] == 0:
            model.update_trained_users()
        elif p["gru"] == 1:
            model.update_trained_users(torch.cat([model.predict_device(se) for se in ses_pred]))
        elif p["gru"] == 3:                                         # :293-300
            model.update_trained_dists()
            model.update_trained_users(torch.cat([model.predict_device(se) for se in ses_pred]))
        else:
            model.update_trained_dists()
            hs, ss = zip(*[model.predict_device(se) for se in ses_pred])
            model.update_trained_users(torch.cat(hs))
            model.update_trained_sus(torch.cat(ss))
        t2 = time.time()
        m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))
        t3 = time.time()
        history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall=[m["at"][k]["recall"] for k in p["at_nums"]],
                            times=(t1 - t0, t2 - t1, t3 - t2)))
        log("epoch %d  sum_loss = %.3f = %.3f + %.3f  auc %.4f  recall@%d %.4f  time (train, user, test) %.2fs %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1, t3 - t2))
        if p["gru"] == 2 and p.get("save_per_epoch", 0) and epoch % p["save_per_epoch"] == 0 and epoch != 0:      # :320-330
            save_checkpoint(model, checkpoint_path(p, model.__class__.__name__, epoch, p.get("model_root", "./model")))
    return model, best, history


def minibatch_default_params():
    """Config of the mini-batch classes of public/GRU.py (`Gru` :395, `Lstm` :502, `Rnn` :661).  The reference has no driver for them
    (its `main`, :813-814, is a stub): the values are default_params()'s with a train batch; `cell` picks the class - "gru", "lstm"
    or "rnn".  The batch cost averages the loss gradients over the batch, so a batch of B users moves 1 / B as far per user as the
    one-by-one drivers do at the same alpha."""
    return dict(at_nums=[5, 10, 15, 20], epochs=3, latent_size=20, alpha=0.01, **{"lambda": 0.001}, cell="lstm",
                batch_size_train=16, batch_size_test=32, seed=123, dataset="synthetic", UD=40, dd=200)


MINIBATCH_CELLS = {"gru": "Gru", "lstm": "Lstm", "rnn": "Rnn"}


def train_minibatch(ds, p=None, device="cuda:0", log=print):
    """train_valid_or_test's epoch for the mini-batch classes: negative refresh -> shuffled users in batches of p["batch_size_train"]
    (one SGD step each) -> snapshot -> predict -> update_trained_users -> evaluate.  -> (model, best, history)."""
    q = minibatch_default_params()
    q.update(p or {})
    p = q
    if p["cell"] not in MINIBATCH_CELLS:
        raise ValueError("p['cell'] must be one of %s (got %r)" % (sorted(MINIBATCH_CELLS), p["cell"]))
    if ds is None or isinstance(ds, str):
        if isinstance(ds, str):
            p = dict(p, dataset=ds)
        ds = load_dataset(p)
    size = p["latent_size"]
    model = getattr(models, MINIBATCH_CELLS[p["cell"]])(train=ds.shard(), test=None, alpha_lambda=[p["alpha"], p["lambda"]], n_user=ds.n_user,
                                                        n_item=ds.n_item, n_in=size, n_hidden=size, device=device, seed=p.get("seed"))
    best = GlobalBest(p["at_nums"])
    U, B = ds.n_user, max(1, int(p["batch_size_train"]))
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    ses_pred = compute_start_end(U, max(int(p["batch_size_test"]), 16384))
    tes_p, tes_m = ds.tes_p.reshape(-1, 1), np.ones((U, 1), np.int32)
    history = []
    for epoch in range(p["epochs"]):
        if epoch > 0:
            model.resample_negatives_device(p.get("seed", 0) * 1000003 + epoch)
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U).astype(np.int32)
        outs = [model.train_batch(order[b0:b0 + B], sync=False) for b0 in range(0, U, B)]
        loss = float(torch.cat(outs).double().sum().item())
        if model.ctx.take_bad_ids(model._stream().value):
            raise IndexError("an index table holds an id outside the model's tables")
        l2 = model.l2.eval()
        t1 = time.time()
        model.update_trained_items()
        model.update_trained_users(torch.cat([model.predict_device(se) for se in ses_pred]))
        t2 = time.time()
        m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))
        t3 = time.time()
        history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall=[m["at"][k]["recall"] for k in p["at_nums"]],
                            times=(t1 - t0, t2 - t1, t3 - t2)))
        log("epoch %d  sum_loss = %.3f = %.3f + %.3f  auc %.4f  recall@%d %.4f  time (train, user, test) %.2fs %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1, t3 - t2))
    return model, best, history


def cal_s(ds, p, device="cuda:0", out_root="./Lmdd", log=print):
    """Mode 's' of the reference driver (prog_bpr_gru_spatial.py:337-362): build the Distance2Pre model, load the checkpoint of
    p['load_epoch'], snapshot the tables, predict every user and save the (n_user, n_dist + 1) bin probabilities `sts` with np.save under
    ./Lmdd/<dataset>_size<D>_UD<UD>_dd<dd>_epoch<e>last1(.npy).  Returns (path, sts)."""
    if p["gru"] != 2:
        raise ValueError("cal_s is the Distance2Pre (gru = 2) mode of the reference driver")
    model = build_model(ds, p, device, seed=p.get("seed"))
    path = checkpoint_path(p, model.__class__.__name__, p["load_epoch"], p.get("model_root", "./model"))
    log("Loading model ...")
    load_checkpoint(model, path)
    log("\tPredicting ...")
    model.update_trained_items(); model.update_trained_dists()
    all_sus = []
    for se in compute_start_end(ds.n_user, max(int(p["batch_size_test"]), 16384)):          # (:354-356; rows are the same for any chunking)
        all_sus.append(model.predict_device(se)[1])
    sts = torch.cat(all_sus).cpu().numpy()
    os.makedirs(out_root, exist_ok=True)
    out = os.path.join(out_root, "%s_size%s_UD%s_dd%s_epoch%slast1" % (p["dataset"], p["latent_size"], p["UD"], p["dd"], p["load_epoch"]))
    np.save(out, sts)
    return out + ".npy", sts


def fpmc_default_params():
    """The in-source config of prog_fpmc_lr.py:55-73 (+ `batch`: transitions per launch - 1 is the reference's one-by-one training -, seed)."""
    return dict(at_nums=[5, 10, 15, 20], epochs=200, latent_size=20, alpha=0.01, **{"lambda": 0.001}, UD=20, batch_size_train=1,
                batch_size_test=32, batch=1, seed=123)


def train_fpmc_lr(ds, p=None, device="cuda:0", log=print):
    """train_valid_or_test of prog_fpmc_lr.py:149-216 on a PoiDataset: OboFpmc_lr over ds (neighbour sets within p['UD'] km built on the
    device), then per epoch: new test negatives (epoch > 0), users shuffled, every transition (u, p[t-1], p[t], one neighbour of p[t]) trained
    in launches of p['batch'] transitions, the sum_loss line (sum of log sigmoid, l2 = model.l2), AUC / top-K metrics into GlobalBest.
    Returns (model, best, history)."""
    p = dict(fpmc_default_params(), **(p or {}))
    tab = ds.shard()
    model = models.OboFpmc_lr(train=tab, test=None, alpha_lambda=[p["alpha"], p["lambda"]], n_user=ds.n_user, n_item=ds.n_item,
                              n_size=p["latent_size"], device=device, seed=p.get("seed"), coords=ds.coords, ud_km=p["UD"])
    best = GlobalBest(p["at_nums"])
    U = ds.n_user
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    tes_p, tes_m = ds.tes_p.reshape(-1, 1), np.ones((U, 1), np.int32)
    B = max(1, int(p.get("batch", 1)))
    history = []
    for epoch in range(p["epochs"]):
        if epoch > 0:                                               # :171-174
            model.resample_test_negatives_device(p.get("seed", 0) * 1000003 + epoch)
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U)   # :179-181
        u, a, i, j = model.epoch_transitions(p.get("seed", 0) * 7919 + epoch, order)
        n = u.numel()
        loss = 0.0
        if B == 1:                                                  # :182-190, one transition per call
            hu, ha, hi, hj = (t.cpu().numpy() for t in (u, a, i, j))
            for t in range(n):
                loss += model.train(int(hu[t]), int(ha[t]), int(hi[t]), [int(hj[t])])
        else:
            parts = [model.train_batch(u[s:s + B], a[s:s + B], i[s:s + B], j[s:s + B], sync=False) for s in range(0, n, B)]
            if model.ctx.take_bad_ids(model._stream().value):
                raise IndexError("rejected transitions in epoch %d" % epoch)
            loss = float(torch.cat(parts).double().sum().item()) if parts else 0.0
        l2 = model.l2.eval()                                        # :191
        t1 = time.time()
        m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))      # :199-201
        t2 = time.time()
        history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall={k: m["at"][k]["recall"] for k in p["at_nums"]},
                            transitions=n, times=(t1 - t0, t2 - t1)))
        log("epoch %d  sum_loss = %.3f = %.3f - %.3f  auc %.4f  recall@%d %.4f  time (train, test) %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1))
    return model, best, history


def prme_default_params():
    """The in-source config of prog_prme.py:44-63 (+ `batch`: transitions per launch - 1 is the reference's one-by-one training -, seed)."""
    return dict(mode="test", split=[0.8, 1.0], at_nums=[5, 10, 15, 20], epochs=100, threshold=360, component_weight=0.2, latent_size=20,
                alpha=0.01, **{"lambda": 0.001}, mini_batch=0, prme=0, batch_size_train=1, batch_size_test=20, batch=1, seed=123)


def train_prme(ds, p=None, device="cuda:0", log=print):
    """train_valid_or_test of prog_prme.py:151-232 on a data.PrmeDataset: OboPrme (OboPRPRM with p['prme'] = 1), then per epoch: new
    negatives on the device (epoch > 0), users shuffled, every transition (u, [tra[i], neg[i], tra[i-1]], dist[i], gap[i]) trained in launches
    of p['batch'], the sum_loss line (sum of log sigmoid + l2), update_trained_items, AUC (always 0, as the reference) and top-K metrics into
    GlobalBest.  Returns (model, best, history)."""
    p = dict(prme_default_params(), **(p or {}))
    cls = models.OboPRPRM if p.get("prme", 0) else models.OboPrme
    model = cls(train=ds, test=None, alpha_lambda=[p["alpha"], p["lambda"]], threshold=p["threshold"], component_weight=p["component_weight"],
                cordi=ds.coords, n_user=ds.n_user, n_item=ds.n_item, n_size=p["latent_size"], device=device, seed=p.get("seed"))
    best = GlobalBest(p["at_nums"])
    U = ds.n_user
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    tes_p, tes_m = np.asarray(ds.tes_p), np.asarray(ds.tes_mask)
    B = max(1, int(p.get("batch", 1)))
    history = []
    for epoch in range(p["epochs"]):
        if epoch > 0:                                               # :179-182
            model.resample_negatives_device(p.get("seed", 0) * 1000003 + epoch)
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U)   # :188-190
        u, pp, q, pv, d, g = model.epoch_transitions(None, order)
        n = u.numel()
        loss = 0.0
        if B == 1:                                                  # :191-197, one transition per call
            hu, hp, hq, hv, hd, hg = (t.cpu().numpy() for t in (u, pp, q, pv, d, g))
            for t in range(n):
                loss += model.train(int(hu[t]), [int(hp[t]), int(hq[t]), int(hv[t])], float(hd[t]), int(hg[t]))
        else:
            parts = [model.train_batch(u[s:s + B], pp[s:s + B], q[s:s + B], pv[s:s + B], d[s:s + B], g[s:s + B], sync=False) for s in range(0, n, B)]
            if model.ctx.take_bad_ids(model._stream().value):
                raise IndexError("rejected transitions in epoch %d" % epoch)
            loss = float(torch.cat(parts).double().sum().item()) if parts else 0.0
        l2 = model.l2.eval()                                        # :199
        t1 = time.time()
        model.update_trained_items()                                # :208
        m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))      # :213-214
        t2 = time.time()
        history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall={k: m["at"][k]["recall"] for k in p["at_nums"]},
                            transitions=n, times=(t1 - t0, t2 - t1)))
        log("epoch %d  sum_loss = %.3f = %.3f + %.3f  auc %.4f  recall@%d %.4f  time (train, test) %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1))
    return model, best, history


def vbpr_default_params():
    """Config of OboVBpr (public/BPR.py:245-335) in the shape of default_params(): the reference has no driver that builds it (nothing
    there loads a feature file).  `launch`: triples per launch (1 = the reference's one-by-one training); `cap`: the batch rule's cap for
    launches of more than one triple; n_img / fea_scale: the synthetic feature table (data.synthetic_features) used when the dataset
    brings none (ds.fea_img)."""
    return dict(at_nums=[5, 10, 15, 20], epochs=3, latent_size=20, alpha=0.01, **{"lambda": 0.001}, lambda_ev=0.001, fea_random_zero=0.0,
                n_img=1024, fea_scale=None, launch=4096, cap=8.0, batch_size_test=32, seed=123, dataset="synthetic", UD=40, dd=200)


def train_vbpr(ds, p=None, device="cuda:0", log=print):
    """The flag-0 epoch of prog_bpr_gru_spatial.py:219-303 for OboVBpr: new negatives on the device (epoch > 0) -> the epoch's triples
    shuffled -> launches of p["launch"] triples -> sum_loss line -> update_trained_items / _users -> AUC and top-K metrics on the
    device.  -> (model, best, history)."""
    from . import data as pdata
    q = vbpr_default_params()
    q.update(p or {})
    p = q
    if ds is None or isinstance(ds, str):
        if isinstance(ds, str):
            p = dict(p, dataset=ds)
        ds = load_dataset(p)
    fea = getattr(ds, "fea_img", None)
    if fea is None:
        fea = pdata.synthetic_features(ds.n_item, p["n_img"], p.get("seed", 0), p.get("fea_scale"))
    size = p["latent_size"]
    model = models.OboVBpr(train=ds.shard(), test=None, alpha_lambda=[p["alpha"], p["lambda"], p["lambda_ev"], p["fea_random_zero"]],
                           n_user=ds.n_user, n_item=ds.n_item, n_in=size, n_hidden=size, n_img=fea.shape[1], fea_img=fea, device=device,
                           seed=p.get("seed"))
    best = GlobalBest(p["at_nums"])
    U, B = ds.n_user, max(1, int(p["launch"]))
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    tes_p, tes_m = ds.tes_p.reshape(-1, 1), np.ones((U, 1), np.int32)
    history = []
    model.ctx.set_batch_cap(float(p["cap"]))
    try:
        for epoch in range(p["epochs"]):
            if epoch > 0:
                model.resample_negatives_device(p.get("seed", 0) * 1000003 + epoch)
            t0 = time.time()
            u, pp, qq = model.epoch_triples()
            gen = torch.Generator(device="cpu").manual_seed(123 + epoch)
            order = torch.randperm(u.numel(), generator=gen).to(model.device)
            u, pp, qq = (t.index_select(0, order).contiguous() for t in (u, pp, qq))
            outs = [model.train_batch(u[s:s + B], pp[s:s + B], qq[s:s + B], sync=False) for s in range(0, u.numel(), B)]
            loss = float(torch.cat(outs).double().sum().item())
            if model.ctx.take_bad_ids(model._stream().value):
                raise IndexError("an index table holds an id outside the model's tables, or a negative equal to its positive")
            l2 = model.l2.eval()
            t1 = time.time()
            model.update_trained_items()
            model.update_trained_users()
            t2 = time.time()
            m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))
            t3 = time.time()
            history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall=[m["at"][k]["recall"] for k in p["at_nums"]],
                                times=(t1 - t0, t2 - t1, t3 - t2)))
            log("epoch %d  sum_loss = %.3f = %.3f + %.3f  auc %.4f  recall@%d %.4f  time (train, user, test) %.2fs %.2fs %.2fs"
                % (epoch, loss + l2, loss, l2, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1, t3 - t2))
    finally:
        model.ctx.set_batch_cap(1.0)
    return model, best, history


def geoie_default_params():
    """The in-source config of prog_geoie.py:46-63 (+ `batch`: users per launch - 1 is the reference's one-by-one training -, seed, d_min (km,
    0 = the reference) and score_norm ("reference" | "count"))."""
    return dict(dataset="Foursquare.txt", mode="test", load_epoch=0, save_per_epoch=100, split=-1, at_nums=[5, 10, 15, 20], epochs=101,
                latent_size=20, alpha=0.01, **{"lambda": 0.001}, mini_batch=0, GeoIE=1, batch_size_train=1, batch_size_test=5, batch=1, seed=123,
                d_min=0.0, score_norm="reference")


def train_geoie(ds, p=None, device="cuda:0", log=print):
    """train_valid_or_test of prog_geoie.py:138-236 on a PoiDataset: OboGeoIE over ds, then per epoch: new negatives on the device (epoch > 0),
    users shuffled, launches of p['batch'] users, the sum_loss line (sum of log sigmoid + l2), update_trained, AUC (always 0, as the
    reference) and top-K metrics into GlobalBest.  The history records a, b and the users rejected in the epoch (logged, not raised: they
    depend on data and parameters; their losses are left out of the sum).  Returns (model, best, history)."""
    p = dict(geoie_default_params(), **(p or {}))
    model = models.OboGeoIE(train=ds.shard(), test=None, alpha_lambda=[p["alpha"], p["lambda"]], n_user=ds.n_user, n_item=ds.n_item,
                            n_in=p["latent_size"], n_hidden=p["latent_size"], coords=ds.coords, device=device, seed=p.get("seed"),
                            d_min=p["d_min"], score_norm=p["score_norm"])
    best = GlobalBest(p["at_nums"])
    U = ds.n_user
    ses_tes = compute_start_end(U, p["batch_size_test"])
    ses_auc = compute_start_end(U, p["batch_size_test"] * 10)
    tes_p, tes_m = ds.tes_p.reshape(-1, 1), np.ones((U, 1), np.int32)
    B = max(1, int(p.get("batch", 1)))
    history = []
    for epoch in range(p["epochs"]):
        if epoch > 0:                                               # :162-167
            model.resample_negatives_device(p.get("seed", 0) * 1000003 + epoch)
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U)   # :175-177
        model.ctx.take_bad_ids(model._stream().value)
        parts = [model.train_batch(order[s:s + B], sync=False) for s in range(0, U, B)]      # :178-185 (B = 1: one user per call)
        rejected = model.ctx.take_bad_ids(model._stream().value)
        model.rejected += rejected
        losses = torch.cat(parts).double() if parts else torch.zeros(0, dtype=torch.float64)
        loss = float(torch.nan_to_num(losses, nan=0.0).sum().item())
        l2 = model.l2.eval()                                        # :186
        a, b = float(model.ab[0].item()), float(model.ab[1].item())
        t1 = time.time()
        model.update_trained()                                      # :200
        m = evaluate_epoch(p, model, best, epoch, ses_auc, ses_tes, tes_p, tes_m, full_rank=bool(p.get("full_rank", False)))      # :204-206
        t2 = time.time()
        history.append(dict(_full_rank(m), epoch=epoch, loss=loss, l2=l2, auc=m["auc"], recall={k: m["at"][k]["recall"] for k in p["at_nums"]},
                            a=a, b=b, rejected=rejected, times=(t1 - t0, t2 - t1)))
        log("epoch %d  sum_loss = %.3f = %.3f + %.3f  a %.6f  b %.6f  rejected users %d  auc %.4f  recall@%d %.4f  time (train, test) %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, a, b, rejected, m["auc"], p["at_nums"][-1], m["at"][p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1))
    return model, best, history


def poi2vec_default_params():
    """The in-source config of prog_poi2vec.py:46-66 (+ `batch`: users per launch - 1 is the reference's one-by-one training -, seed, and the
    two scoring switches of models.OboPoi2vec, default = what the reference computes)."""
    return dict(dataset="Gowalla.txt", mode="test", regionThreshold=0.1, timeThreshold=360, split=[0.8, 1.0], at_nums=[5, 10, 15, 20], epochs=100,
                latent_size=20, initial_alpha=1, initial_loss=25000, alpha=0.01, **{"lambda": 0.001}, mini_batch=0, poi2vec=0,
                batch_size_train=4, batch_size_test=25, batch=1, seed=123, softmax_axis="reference", eval_context="reference")


def poi2vec_model(ds, p=None, device="cuda:0"):
    """build_model_one_by_one of prog_poi2vec.py:92-113 on a data.Poi2vecDataset (alpha starts at initial_alpha)."""
    p = dict(poi2vec_default_params(), **(p or {}))
    return models.OboPoi2vec(train=ds, test=None, alpha_lambda=[p["initial_alpha"], p["lambda"]], n_user=ds.n_user, n_item=ds.n_item,
                             n_node=ds.n_node, n_size=p["latent_size"], probs=ds.probs, routes=ds.routes, lrs=ds.lrs, device=device,
                             seed=p.get("seed"), softmax_axis=p["softmax_axis"], eval_context=p["eval_context"])


def poi2vec_recall(model, ds, p, at_nums):
    """The top-K metrics of Valuate.py:132-191 over batches of p['batch_size_test'] users, batch by batch (with softmax_axis 'reference' the
    scores depend on the batch: the ranges are not merged), accumulated on the device (poi_rank_metrics)."""
    from .evaluate import device_rank_metrics
    p = dict(poi2vec_default_params(), **(p or {}))
    if model.tes_len_max != 1:
        raise ValueError("the evaluation expects one test position per user (split [.., 1.0]); found %d" % model.tes_len_max)
    tot = None
    for se in compute_start_end(ds.n_user, p["batch_size_test"]):
        m = device_rank_metrics(model, [se], at_nums)
        if tot is None:
            tot = {k: dict(hits=0.0, map=0.0, ndcg=0.0) for k in at_nums}
        for k in at_nums:
            tot[k]["hits"] += m[k]["hits"]; tot[k]["map"] += m[k]["map"] * model.n_user; tot[k]["ndcg"] += m[k]["ndcg"] * model.n_user
    denom = float(model.tes_masks.sum().item())
    out = {}
    for k in at_nums:
        rec, pre = tot[k]["hits"] / denom, tot[k]["hits"] / (k * model.n_user)
        out[k] = dict(hits=tot[k]["hits"], recall=rec, precision=pre, f1=2.0 * rec * pre / (rec + pre) if rec + pre > 0 else 0.0,
                      map=tot[k]["map"] / model.n_user, ndcg=tot[k]["ndcg"] / model.n_user)
    return out


def train_poi2vec(ds, p=None, device="cuda:0", log=print):
    """train_valid_or_test of prog_poi2vec.py:138-207 on a data.Poi2vecDataset: OboPoi2vec at alpha = initial_alpha, then per epoch: users
    shuffled, launches of p['batch'] users, the sum_loss line (sum of upq + l2), update_trained_params, AUC (always 0, as the reference)
    and the top-K metrics into GlobalBest; after the epoch alpha is divided by 10 when the epoch loss rose above the previous one (the
    first comparison is against initial_loss) and alpha >= 10 p['alpha'] (:196-199).  Rejected users are logged, not raised; their losses
    are left out of the sum.  Returns (model, best, history)."""
    p = dict(poi2vec_default_params(), **(p or {}))
    model = poi2vec_model(ds, p, device)
    best = GlobalBest(p["at_nums"])
    U = ds.n_user
    B = max(1, int(p.get("batch", 1)))
    pre_loss, lr_min = float(p["initial_loss"]), float(p["alpha"])
    history = []
    for epoch in range(p["epochs"]):
        t0 = time.time()
        order = np.random.default_rng(123 + epoch).permutation(U)   # :158-161
        model.ctx.take_bad_ids(model._stream().value)
        parts = [model.train_batch(order[s:s + B], sync=False) for s in range(0, U, B)]      # :162-164 (B = 1: one user per call)
        rejected = model.ctx.take_bad_ids(model._stream().value)
        model.rejected += rejected
        losses = torch.cat(parts).double() if parts else torch.zeros(0, dtype=torch.float64)
        loss = float(torch.nan_to_num(losses, nan=0.0).sum().item())
        l2 = model.l2.eval()                                        # :165
        t1 = time.time()
        model.update_trained_params()                               # :173
        at = poi2vec_recall(model, ds, p, p["at_nums"])            # :178-180
        for i, k in enumerate(p["at_nums"]):
            for name, key in (("recall", "recall"), ("precis", "precision"), ("f1scor", "f1"), ("map", "map"), ("ndcg", "ndcg")):
                cur = getattr(best, "best_" + name)
                if at[k][key] > cur[i]:
                    cur[i] = at[k][key]
                    getattr(best, "best_epoch_" + name)[i] = epoch
        t2 = time.time()
        lr = model.alpha_lambda[0]
        history.append(dict(epoch=epoch, loss=loss, l2=l2, auc=0.0, recall={k: at[k]["recall"] for k in p["at_nums"]}, alpha=lr,
                            rejected=rejected, times=(t1 - t0, t2 - t1)))
        log("epoch %d  sum_loss = %.3f = %.3f + %.3f  alpha %g  rejected users %d  auc %.4f  recall@%d %.4f  time (train, test) %.2fs %.2fs"
            % (epoch, loss + l2, loss, l2, lr, rejected, 0.0, p["at_nums"][-1], at[p["at_nums"][-1]]["recall"], t1 - t0, t2 - t1))
        if pre_loss < loss and lr >= lr_min * 10:                   # :196-198
            model.alpha_lambda = [lr / 10, p["lambda"]]
        pre_loss = loss
    return model, best, history


def serve_replay(model, ds=None, k=20):
    """Online use of a trained recurrent model (models.Session for the GRU family, models.CellSession - model.cell_session() - for Lstm,
    Rnn and OboCARNN): seed every user's state from the training rows (`load_history`),
    advance every user by their first held-out test POI as if it had just been checked in, and recommend the next top-k from the new
    state.  `ds` is the data set the model was built from (its tables already live in the model; accepted for symmetry with the
    train_* drivers).  Returns (session, (n_user, k) int32 device indices)."""
    s = model.cell_session() if hasattr(model, "cell_session") else model.session()
    s.load_history()
    users = np.arange(model.n_user)
    tes = model.tes_buys_masks[:, 0].cpu().numpy()
    ok = (model.tes_masks[:, 0].cpu().numpy() > 0) & (tes < model.n_item)
    s.advance(users[ok], tes[ok])
    return s, s.recommend(users, k)
