#!/usr/bin/env python
"""Generate tests/golden/fpmc_neighbors.npz.  Run ONLY where the reference checkout is available (its path is the first argument,
default ../reference next to the repository).

Records the reference's own FPMC-LR neighbour sets (public/Load_Data_fpmc_lr.py:114-143, fun_acquire_neighbors_for_each_poi, which runs
under Python 3) at UD = 20 km for two coordinate sets:
  * "small": the 45 POIs of sequences_small.txt, in the order data.load_sequence_file numbers them (the coordinate array is passed
    directly: the reference's own aliasing goes through a set() of strings and depends on the hash seed);
  * "hard": ~1500 coordinates - clusters, exact duplicates, and pairs placed within a few float64 steps of the 20 km boundary in
    several directions and latitudes (the cases where a distance computed in a different operation order would flip).
Only arrays are written; no reference source text is stored.
"""
import math
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import public.Load_Data_fpmc_lr as LF           # noqa: E402  (reference, read-only)
import poi_amd                                  # noqa: E402
from poi_amd import data as D                   # noqa: E402

UD = 20.0


def ref_csr(coords):
    nb = LF.fun_acquire_neighbors_for_each_poi([list(map(float, c)) for c in coords], UD)
    n = len(coords)
    rows = [sorted(int(k) for k in nb.get(i, [])) for i in range(n)]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([k for r in rows for k in r], np.int32)
    return off, ids


def boundary_points(lat0, lon0, dlat, dlon):
    """Points p(t) = (lat0 + t dlat, lon0 + t dlon): the float64 step of t at which the reference's cal_dis from (lat0, lon0) passes UD,
    then the coordinates 3 float64 steps (of the moving coordinate) either side of it."""
    def dist(lat, lon):
        return LF.cal_dis(lat0, lon0, lat, lon)
    lo, hi = 0.0, 1.0
    while dist(lat0 + hi * dlat, lon0 + hi * dlon) <= UD:
        hi *= 2
    for _ in range(200):
        mid = (lo + hi) / 2
        if mid in (lo, hi):
            break
        if dist(lat0 + mid * dlat, lon0 + mid * dlon) <= UD:
            lo = mid
        else:
            hi = mid
    lat, lon = lat0 + hi * dlat, lon0 + hi * dlon
    out = []
    for s in range(-3, 4):
        if dlon != 0.0:
            b = struct.unpack("<q", struct.pack("<d", lon))[0] + s
            out.append((lat, struct.unpack("<d", struct.pack("<q", b))[0]))
        else:
            b = struct.unpack("<q", struct.pack("<d", lat))[0] + s
            out.append((struct.unpack("<d", struct.pack("<q", b))[0], lon))
    return out


def hard_coords(rng):
    pts = []
    # clusters: 900 points in 12 clusters of ~5-30 km radius spread over ~300 km
    centres = np.stack([40.0 + rng.uniform(0, 2.7, 12), -74.0 + rng.uniform(0, 3.5, 12)], 1)
    for c in centres:
        r = rng.uniform(0.05, 0.3)
        m = 75
        pts += list(zip(c[0] + rng.normal(0, r, m), c[1] + rng.normal(0, r * 1.3, m)))
    # exact duplicates of 60 of them
    dup = rng.choice(len(pts), 60, replace=False)
    pts += [pts[i] for i in dup]
    # near-boundary pairs: latitudes 0 .. 70, four directions
    for lat0 in (0.3, 23.5, 40.7, 55.1, 69.8, -33.9):
        lon0 = float(rng.uniform(-170, 170))
        pts.append((lat0, lon0))
        for dlat, dlon in ((1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-0.3, 0.95), (-1.0, 0.0)):
            pts += boundary_points(lat0, lon0, dlat, dlon)
    # filler: uniform over a 300 km box
    while len(pts) < 1500:
        pts.append((float(40.0 + rng.uniform(0, 2.7)), float(-74.0 + rng.uniform(0, 3.5))))
    return np.asarray(pts, np.float64)


def main():
    ds = D.load_sequence_file(os.path.join(HERE, "sequences_small.txt"), split=-1, dd=200, dist_num=200, seed=3)
    small = np.asarray(ds.coords, np.float64)
    hard = hard_coords(np.random.default_rng(20261016))
    out = dict(ud_km=np.float64(UD))
    for name, xy in (("small", small), ("hard", hard)):
        off, ids = ref_csr(xy)
        out[name + "_coords"], out[name + "_off"], out[name + "_ids"] = xy, off, ids
        print(name, len(xy), "points, mean neighbours %.1f" % (off[-1] / len(xy)))
    np.savez_compressed(os.path.join(HERE, "fpmc_neighbors.npz"), **out)


if __name__ == "__main__":
    main()
