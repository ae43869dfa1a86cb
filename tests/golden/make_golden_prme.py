#!/usr/bin/env python
"""Generate tests/golden/prme_load_data.npz (and the valid-mode input prme_valid_small.txt).  Run ONLY where the reference checkout is
available (its path is the first argument, default ../reference next to the repository); it needs pandas and numpy.

Runs the reference's own PRME loading - public/Load_Data_prme.py load_data + fun_data_pois_masks, as prog_prme.py:67-73 calls them - on
  * "test":  sequences_small.txt in test mode (split [0.8, 1.0]);
  * "valid": prme_valid_small.txt in valid mode (split [0.6, 0.8]).  sequences_small.txt itself makes the reference raise KeyError in
    valid mode (a POI seen only in the dropped tail); that is recorded as valid_small_raises = 1.  prme_valid_small.txt is
    sequences_small.txt with every user's first ceil(le / 4) check-ins appended again, so that the dropped tail repeats kept POIs.
Stored per case: the reference's alias order as raw POI ids (ref_ids: alias k <-> raw id), n_user, n_item, location, and the padded
train / test POIs, gaps, distances and masks.  Only arrays are written; no reference source text is stored.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, REF)

import public.Load_Data_prme as LP              # noqa: E402  (reference, read-only)


def make_valid_input(src, dst):
    import pandas as pd
    tab = pd.read_csv(src, sep=" ")
    rows = []
    for _, r in tab.iterrows():
        p, t, c = str(r["u_pois"]).split("/"), str(r["u_times"]).split("/"), str(r["u_coordinates"]).split("/")
        k = int(math.ceil(len(p) / 4.0))
        last = int(float(t[-1]))
        p2, c2 = p + p[:k], c + c[:k]
        t2 = t + [str(last + 10 * (i + 1)) for i in range(k)]
        rows.append((len(p2), r["pois_different"], r["u_id"], "/".join(p2), "/".join(t2), "/".join(c2)))
    cols = ["check_times", "pois_different", "u_id", "u_pois", "u_times", "u_coordinates"]
    pd.DataFrame(rows, columns=cols).to_csv(dst, sep=" ", index=False, columns=cols)


def record(out, name, path, mode, split):
    [(un, itn, loc), (trp, tep), (trt, tet), (trd, ted)] = LP.load_data(path, mode, split)
    # the reference's alias order: recover it from its own output (alias of a raw id = its position in the set iteration)
    import pandas as pd
    tab = pd.read_csv(path, sep=" ")
    raw = [str(s).split("/") for s in tab["u_pois"]]
    ref_ids = np.full(itn, -1, np.int64)
    for u, seq in enumerate(raw):
        le = len(seq)
        kept = seq[:int(le * split[1])]
        for s_, a_ in zip(kept, list(trp[u]) + list(tep[u])):
            ref_ids[a_] = int(s_)
    assert (ref_ids >= 0).all()
    tpm, ttm, tdm, tmk = LP.fun_data_pois_masks(trp, trt, trd, [itn])
    epm, etm, edm, emk = LP.fun_data_pois_masks(tep, tet, ted, [itn])
    out.update({name + "_n_user": np.int64(un), name + "_n_item": np.int64(itn), name + "_location": np.asarray(loc, np.float64),
                name + "_ref_ids": ref_ids, name + "_tra_pois": np.asarray(tpm, np.int64), name + "_tra_times": np.asarray(ttm, np.float64),
                name + "_tra_dists": np.asarray(tdm, np.float64), name + "_tra_masks": np.asarray(tmk, np.int64),
                name + "_tes_pois": np.asarray(epm, np.int64), name + "_tes_masks": np.asarray(emk, np.int64)})


def main():
    small = os.path.join(HERE, "sequences_small.txt")
    vin = os.path.join(HERE, "prme_valid_small.txt")
    make_valid_input(small, vin)
    out = {}
    record(out, "test", small, "test", [0.8, 1.0])
    record(out, "valid", vin, "valid", [0.6, 0.8])
    try:
        LP.load_data(small, "valid", [0.6, 0.8])
        out["valid_small_raises"] = np.int64(0)
    except KeyError:
        out["valid_small_raises"] = np.int64(1)
    np.savez_compressed(os.path.join(HERE, "prme_load_data.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
