#!/usr/bin/env python
"""Generate tests/golden/geoie_pairs.npz.  Run ONLY where the reference checkout is available (its path is the first argument, default
../reference next to the repository); it needs pandas and numpy.

Runs the reference's own GeoIE data path - public/Load_Data_GeoIE.py load_data + fun_data_buys_masks + fun_random_neg_masks_tra (seeded)
+ fun_compute_dist_neg, as prog_geoie.py:70-77 calls them - on sequences_small.txt with split -1 ("s1") and -2 ("s2").  Stored per case:
the reference's alias order as raw POI ids (ref_ids: alias k <-> raw id), n_user, n_item, pois_cordis, the padded train POIs / negatives /
mask, and the distances dp / dq of every row in packed lower-triangular order (row i >= 1 of fun_compute_dist_neg keeps its first i
entries).  Only arrays are written; no reference source text is stored.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, REF)

import public.Load_Data_GeoIE as LG             # noqa: E402  (reference, read-only)


def record(out, name, path, split):
    [(un, itn), cordi, (tra, tes), (trd, ted), cnt] = LG.load_data(path, "test", split)
    import pandas as pd
    raw = [str(s).split("/") for s in pd.read_csv(path, sep=" ")["u_pois"]]
    ref_ids = np.full(itn, -1, np.int64)
    for u, seq in enumerate(raw):
        for s_, a_ in zip(seq[:split] + [seq[split]], list(tra[u]) + list(tes[u])):
            ref_ids[a_] = int(s_)
    tbm, _, tmk, _ = LG.fun_data_buys_masks(tra, trd, [itn], [0], cnt)
    random.seed(7)
    neg = LG.fun_random_neg_masks_tra(itn, tbm)
    pd_, qd_, _ = LG.fun_compute_dist_neg(tbm, tmk, neg, cordi)
    dp, dq = [], []
    for up, uq in zip(pd_, qd_):
        for i, (rp, rq) in enumerate(zip(up, uq)):
            dp.extend(rp[:i + 1]); dq.extend(rq[:i + 1])
    out.update({name + "_n_user": np.int64(un), name + "_n_item": np.int64(itn), name + "_ref_ids": ref_ids,
                name + "_cordi": np.asarray(cordi, np.float64), name + "_tra_buys": np.asarray(tbm, np.int64),
                name + "_tra_neg": np.asarray(neg, np.int64), name + "_tra_masks": np.asarray(tmk, np.int64),
                name + "_dp": np.asarray(dp, np.float64), name + "_dq": np.asarray(dq, np.float64)})


def main():
    small = os.path.join(HERE, "sequences_small.txt")
    out = {}
    record(out, "s1", small, -1)
    record(out, "s2", small, -2)
    np.savez_compressed(os.path.join(HERE, "geoie_pairs.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
