"""Host-side input contract of the hot path (the reference's public/Load_Data_by_length.py), vectorised
with numpy, plus the synthetic Foursquare/Gowalla-shaped generator used by bench.py and the tests.

Layouts follow the reference exactly where the model sees them:
  * padding id = n_item for POIs and dist_num for distance bins (Load_Data_by_length.py:115-124);
  * dist[0] = dist_num for every sequence (:77); bin = min(int(km*1000/dd), dist_num) (:38-39);
  * negatives uniform over [0, n_item) rejecting the user's own train POIs (:127-143);
  * negative distance bin t = bin(neg_t, pos_{t-1}) (:165-180).
On the device nothing is padded: sequences are CSR-packed (off / flat arrays); `to_padded()` rebuilds
the reference's nested-list tables for API compatibility.
"""
from __future__ import annotations

import dataclasses

import numpy as np

EARTH_D = 12742                      # Load_Data_by_length.py:30
DEG = 0.017453292519943295           # :31


def cal_dis_vec(lat1, lon1, lat2, lon2, dd, dist_num):
    """Vectorised public/Load_Data_by_length.py:24-42 (same float64 expression order)."""
    lat1, lon1, lat2, lon2 = (np.asarray(v, np.float64) for v in (lat1, lon1, lat2, lon2))
    a = (lat1 - lat2) * DEG
    b = (lon1 - lon2) * DEG
    c = (1.0 - np.cos(a)) / 2 + np.cos(lat1 * DEG) * np.cos(lat2 * DEG) * (1.0 - np.cos(b)) / 2
    dist = EARTH_D * np.arcsin(np.sqrt(c))
    interval = (dist * 1000 / dd).astype(np.int64)
    return np.minimum(interval, dist_num)


def bin_thresholds(dd, dist_num):
    """thr[k-1] = the smallest float64 c with int(12742*asin(sqrt(c))*1000/dd) >= k, k = 1..dist_num,
    found by bisection on the float64 bit pattern with the SAME libm calls as cal_dis
    (Load_Data_by_length.py:36-38).  Then  bin(c) = #{k : c >= thr[k-1]}  reproduces the reference's
    asin/sqrt/int chain exactly for every c, and the device needs no asin/sqrt at all."""
    import math
    import struct

    def f(c):
        return int(EARTH_D * math.asin(math.sqrt(c)) * 1000 / dd)

    def bits(x):
        return struct.unpack("<q", struct.pack("<d", x))[0]

    def val(b):
        return struct.unpack("<d", struct.pack("<q", b))[0]

    out = np.empty(dist_num, np.float64)
    lo_b = 0
    for k in range(1, dist_num + 1):
        hi = math.sin(min(k * dd / 1000.0 / EARTH_D, math.pi / 2)) ** 2
        hi = min(hi * (1 + 1e-6) + 1e-300, 1.0)
        while f(hi) < k and hi < 1.0:
            hi = min(hi * 1.001, 1.0)
        lo, hb = lo_b, bits(hi)            # f(val(lo)) < k <= f(val(hb))  (lo = previous threshold - works since f is monotone)
        if f(val(lo)) >= k:
            out[k - 1] = val(lo)
            continue
        while hb - lo > 1:
            mid = (lo + hb) // 2
            if f(val(mid)) >= k:
                hb = mid
            else:
                lo = mid
        out[k - 1] = val(hb)
        lo_b = lo
    return out


def cos_lat(coords):
    """cos(lat * pi/180) per POI with the SCALAR libm cos the reference calls (cal_dis :35) - always: numpy's vectorised float64 cos
    is a SIMD routine that is not correctly rounded and may differ from libm in the last bit on rare inputs, and one ulp of cos(lat)
    can flip a distance bin at a threshold.  ~0.15 us per POI (1.5 s at 10 M POIs, once per data set)."""
    import math
    lat = np.asarray(coords)[:, 0].astype(np.float64) * DEG
    return np.fromiter(map(math.cos, lat.tolist()), np.float64, count=len(lat))


def ud_threshold(ud_km):
    """FPMC-LR neighbour radius as a Haversine `c` (public/Load_Data_fpmc_lr.py:25-34, 114-143: neighbour <=> cal_dis <= UD km): the
    smallest float64 c with 12742 * asin(sqrt(c)) > ud_km, found by bisection on the float64 bit pattern with the scalar libm calls of
    cal_dis (as bin_thresholds).  Then  neighbour <=> c < c_ud  for every c, and the device needs no asin / sqrt."""
    import math
    import struct

    def far(c):
        return EARTH_D * math.asin(math.sqrt(c)) > ud_km

    def val(b):
        return struct.unpack("<d", struct.pack("<q", b))[0]

    lo, hi = 0, struct.unpack("<q", struct.pack("<d", 1.0))[0]      # far(val(lo)) is False for ud_km >= 0; far(1.0) unless ud_km >= 20015
    if not far(val(hi)):
        return np.inf
    if far(val(lo)):
        return 0.0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if far(val(mid)):
            hi = mid
        else:
            lo = mid
    return val(hi)


def fpmc_neighbors_host(coords, ud_km, block=2048):
    """neighbours(i) = {k != i : cal_dis(i, k) <= ud_km} (public/Load_Data_fpmc_lr.py:114-143) as CSR: (off int64 (n+1), ids int32),
    each row ascending.  The Haversine c in cal_dis's operation order (cos of the latitudes from cos_lat), compared with ud_threshold.
    numpy's vectorised cos may differ from the scalar libm cos of the reference in the last bit, so every pair whose c lands within
    1e-9 (relative) of the threshold is recomputed with math.cos: the sets equal the reference's on every input.  The CPU checker of
    poi_fpmc_neighbor_counts / _fill."""
    import math
    xy = np.asarray(coords, np.float64)
    n = len(xy)
    c_ud = ud_threshold(ud_km)
    cphi = cos_lat(xy)
    lat, lon = xy[:, 0], xy[:, 1]
    counts, ids = np.zeros(n, np.int64), []
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        a = (lat[r0:r1, None] - lat[None, :]) * DEG
        b = (lon[r0:r1, None] - lon[None, :]) * DEG
        c = (1.0 - np.cos(a)) / 2 + cphi[r0:r1, None] * cphi[None, :] * (1.0 - np.cos(b)) / 2
        near = np.abs(c - c_ud) <= 1e-9 * c_ud
        for q, k in zip(*np.nonzero(near)):
            i = r0 + int(q)
            c[q, k] = (1.0 - math.cos((lat[i] - lat[k]) * DEG)) / 2 + cphi[i] * cphi[k] * (1.0 - math.cos((lon[i] - lon[k]) * DEG)) / 2
        m = c < c_ud
        m[np.arange(r1 - r0), np.arange(r0, r1)] = False
        counts[r0:r1] = m.sum(axis=1)
        ids.append(np.nonzero(m)[1].astype(np.int32))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off, (np.concatenate(ids) if ids else np.zeros(0, np.int32))


def train_exclusion_csr(off, p_flat, n_item):
    """Every user's DISTINCT train POIs as a CSR (off int64 (n_user + 1), ids int32), ids ascending within a row: the exclude="train"
    lists of compute_sub_topk_near.  A padding id (>= n_item) never is a candidate and is dropped."""
    off = np.asarray(off, np.int64)
    p = np.asarray(p_flat, np.int64)
    n_user = len(off) - 1
    user = np.repeat(np.arange(n_user), np.diff(off))
    keep = (p >= 0) & (p < n_item)
    key = np.unique(user[keep] * (n_item + 1) + p[keep])                 # sorted by (user, POI), duplicates dropped
    eo = np.zeros(n_user + 1, np.int64)
    np.cumsum(np.bincount(key // (n_item + 1), minlength=n_user), out=eo[1:])
    if eo[-1] >= 1 << 31:
        raise ValueError("the train exclusion lists hold %d ids: above 2^31" % eo[-1])
    return eo, (key % (n_item + 1)).astype(np.int32)


def visitors_csr(off, p_flat, n_item):
    """Every POI's DISTINCT train visitors as a CSR (voff int64 (n_item + 1), users int32), user ids ascending within a POI: the inverse
    of train_exclusion_csr and the exclude="train" lists of recommend_audience.  A padding id (>= n_item) is no visit."""
    off = np.asarray(off, np.int64)
    p = np.asarray(p_flat, np.int64)
    n_user = len(off) - 1
    user = np.repeat(np.arange(n_user), np.diff(off))
    keep = (p >= 0) & (p < n_item)
    key = np.unique(p[keep] * max(n_user, 1) + user[keep])                # sorted by (POI, user), duplicates dropped
    voff = np.zeros(n_item + 1, np.int64)
    np.cumsum(np.bincount(key // max(n_user, 1), minlength=n_item), out=voff[1:])
    if voff[-1] >= 1 << 31:
        raise ValueError("the visitor lists hold %d ids: above 2^31" % voff[-1])
    return voff, (key % max(n_user, 1)).astype(np.int32)


def group_exclusion_csr(ex_off, ex_ids, g_off, g_mem, n_item):
    """One exclusion list per GROUP from per-user lists: the sorted union of the members' lists, as a CSR (off int64 (n_grp + 1), ids
    int32) - with (ex_off, ex_ids) = train_exclusion_csr(...) the exclude="train" lists of recommend_group: a POI any member has visited
    leaves the group's ranking.  g_off (n_grp + 1) ascending offsets from 0 into g_mem (ValueError), g_mem user ids inside the per-user
    CSR (IndexError); a user listed twice counts once, an empty group gets an empty list."""
    eo = np.asarray(ex_off, np.int64).reshape(-1)
    ex = np.asarray(ex_ids, np.int64).reshape(-1)
    go = np.asarray(g_off, np.int64).reshape(-1)
    gm = np.asarray(g_mem, np.int64).reshape(-1)
    if len(go) < 1 or go[0] != 0 or go[-1] != len(gm) or np.any(np.diff(go) < 0):
        raise ValueError("g_off must hold ascending offsets from 0 to len(g_mem) = %d" % len(gm))
    if gm.size and (gm.min() < 0 or gm.max() >= len(eo) - 1):
        raise IndexError("group members must lie in [0, %d) (found %d..%d)" % (len(eo) - 1, int(gm.min()), int(gm.max())))
    n_grp = len(go) - 1
    grp = np.repeat(np.arange(n_grp), np.diff(go))                        # the group of every member occurrence
    beg, ln = eo[gm], eo[gm + 1] - eo[gm]
    pos = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln - beg, ln)
    key = np.unique(np.repeat(grp, ln) * (n_item + 1) + ex[pos])          # sorted by (group, POI), duplicates dropped
    off = np.zeros(n_grp + 1, np.int64)
    np.cumsum(np.bincount(key // (n_item + 1), minlength=n_grp), out=off[1:])
    if off[-1] >= 1 << 31:
        raise ValueError("the group exclusion lists hold %d ids: above 2^31" % off[-1])
    return off, (key % (n_item + 1)).astype(np.int32)


def last_exclusion_csr(anchor):
    """exclude="last" as a CSR: row r lists anchor[r] alone; a row without an anchor (-1) excludes nothing."""
    a = np.asarray(anchor, np.int64).reshape(-1)
    off = np.zeros(len(a) + 1, np.int64)
    np.cumsum(a >= 0, out=off[1:])
    return off, a[a >= 0].astype(np.int32)


def check_exclusion_csr(off, ids, n, n_item):
    """Range- and order-check host exclusion lists for n rows -> (off int32 (n + 1), ids int32).  off ascends from 0 to len(ids)
    (ValueError); ids lie in [0, n_item) (IndexError) and are strictly ascending - sorted, unique - within every row (ValueError): the
    kernel finds an id by binary search."""
    off = np.asarray(off, np.int64).reshape(-1)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if len(off) != n + 1 or off[0] != 0 or off[-1] != len(ids) or np.any(np.diff(off) < 0):
        raise ValueError("exclude=(off, ids): off must hold n + 1 = %d ascending offsets from 0 to len(ids) = %d" % (n + 1, len(ids)))
    if ids.size and (ids.min() < 0 or ids.max() >= n_item):
        raise IndexError("exclude ids must lie in [0, %d) (found %d..%d)" % (n_item, int(ids.min()), int(ids.max())))
    if ids.size > 1:
        inner = np.ones(len(ids) - 1, bool)
        cut = off[1:-1]
        inner[cut[(cut > 0) & (cut < len(ids))] - 1] = False               # neighbours that belong to two rows
        if np.any((np.diff(ids) <= 0) & inner):
            raise ValueError("exclude ids must be strictly ascending (sorted, unique) within every row")
    return off.astype(np.int32), ids.astype(np.int32)


def padded_to_csr(rows, lens):
    """Nested (U, LM) table + valid lengths -> (off int32 (U+1), flat int32)."""
    rows = np.asarray(rows)
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    mask = np.arange(rows.shape[1])[None, :] < lens[:, None]
    return off.astype(np.int32), np.ascontiguousarray(rows[mask], dtype=np.int32)


def csr_to_padded(off, flat, pad, len_max=None):
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    lm = int(lens.max()) if len_max is None else int(len_max)
    out = np.full((len(lens), lm), pad, np.int32)
    mask = np.arange(lm)[None, :] < lens[:, None]
    out[mask] = flat
    return out


def sample_negatives(rng, n_item, off, pos_flat, exclude_off=None, exclude_flat=None):
    """One uniform negative per position, rejecting the user's own items
    (fun_random_neg_masks_tra :127-143; with exclude_* also the test items, _tes :146-162)."""
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    user_of = np.repeat(np.arange(len(lens)), lens)
    stride = np.int64(n_item) + 1
    own = user_of * stride + np.asarray(pos_flat, np.int64)
    if exclude_flat is not None:
        eoff = np.asarray(exclude_off, np.int64)
        euser = np.repeat(np.arange(len(eoff) - 1), np.diff(eoff))
        own = np.concatenate((own, euser * stride + np.asarray(exclude_flat, np.int64)))
    own = np.unique(own)
    return own, user_of, stride


def random_neg_tra(rng, n_item, off, p_flat):
    own, user_of, stride = sample_negatives(rng, n_item, off, p_flat)
    neg = rng.integers(0, n_item, size=len(p_flat), dtype=np.int64)
    bad = np.isin(user_of * stride + neg, own, assume_unique=False)
    while bad.any():
        neg[bad] = rng.integers(0, n_item, size=int(bad.sum()), dtype=np.int64)
        bad[bad] = np.isin(user_of[bad] * stride + neg[bad], own)
    return neg.astype(np.int32)


def random_neg_tes(rng, n_item, tra_off, tra_flat, tes_off, tes_flat):
    own, _, stride = sample_negatives(rng, n_item, tra_off, tra_flat, tes_off, tes_flat)
    tes_off = np.asarray(tes_off, np.int64)
    user_of = np.repeat(np.arange(len(tes_off) - 1), np.diff(tes_off))
    neg = rng.integers(0, n_item, size=len(tes_flat), dtype=np.int64)
    bad = np.isin(user_of * stride + neg, own)
    while bad.any():
        neg[bad] = rng.integers(0, n_item, size=int(bad.sum()), dtype=np.int64)
        bad[bad] = np.isin(user_of[bad] * stride + neg[bad], own)
    return neg.astype(np.int32)


def dist_neg_bins(off, p_flat, q_flat, coords, dd, dist_num):
    """fun_compute_dist_neg (:165-180): bin(neg_t, pos_{t-1}) for t >= 1, dist_num at t = 0."""
    off = np.asarray(off, np.int64)
    out = np.full(len(p_flat), dist_num, np.int32)
    first = np.zeros(len(p_flat), bool)
    first[off[:-1][np.diff(off) > 0]] = True
    idx = np.nonzero(~first)[0]
    prev = coords[np.asarray(p_flat)[idx - 1]]
    cur = coords[np.asarray(q_flat)[idx]]
    out[idx] = cal_dis_vec(cur[:, 0], cur[:, 1], prev[:, 0], prev[:, 1], dd, dist_num)
    return out


def dist_pos_bins(off, p_flat, coords, dd, dist_num):
    """load_data's train distance sequence (:70-78): bin(pos_t, pos_{t-1}), dist_num at t = 0."""
    off = np.asarray(off, np.int64)
    out = np.full(len(p_flat), dist_num, np.int32)
    first = np.zeros(len(p_flat), bool)
    first[off[:-1][np.diff(off) > 0]] = True
    idx = np.nonzero(~first)[0]
    prev = coords[np.asarray(p_flat)[idx - 1]]
    cur = coords[np.asarray(p_flat)[idx]]
    out[idx] = cal_dis_vec(cur[:, 0], cur[:, 1], prev[:, 0], prev[:, 1], dd, dist_num)
    return out


@dataclasses.dataclass
class CsrTables:
    """Unpadded form of the (train, test, dist) ctor arguments for a user range: what the device holds."""
    off: np.ndarray
    p: np.ndarray
    q: np.ndarray
    dp: np.ndarray
    dq: np.ndarray
    len_max: int               # padded row length the reference would have used (dataset-wide maximum)
    tes_p: np.ndarray          # (n, len_tes)
    tes_q: np.ndarray
    tes_mask: np.ndarray
    tes_dp: np.ndarray

    @property
    def n_user(self):
        return len(self.off) - 1


@dataclasses.dataclass
class PoiDataset:
    """CSR-packed check-in data in the shape Params.__init__ (prog_bpr_gru_spatial.py:49-100) builds."""
    n_user: int
    n_item: int
    dist_num: int
    dd: float
    coords: np.ndarray          # (n_item, 2) float64 lat, lon  (pois_cordis)
    off: np.ndarray             # (n_user+1,) int32
    tra_p: np.ndarray           # flat train POIs
    tra_dp: np.ndarray          # flat train distance bins
    tes_p: np.ndarray           # (n_user,) held-out POI (split = -1)
    tes_dp: np.ndarray          # (n_user,) its distance bin
    tra_q: np.ndarray = None    # flat negatives (resampled per epoch)
    tra_dq: np.ndarray = None   # flat negative distance bins
    tes_q: np.ndarray = None    # (n_user,) test negatives

    @property
    def lens(self):
        return np.diff(np.asarray(self.off, np.int64))

    @property
    def len_max(self):
        return int(self.lens.max())

    def resample_negatives(self, rng):
        """Per-epoch refresh, prog_bpr_gru_spatial.py:221-228."""
        self.tra_q = random_neg_tra(rng, self.n_item, self.off, self.tra_p)
        tes_off = np.arange(self.n_user + 1, dtype=np.int32)
        self.tes_q = random_neg_tes(rng, self.n_item, self.off, self.tra_p, tes_off, self.tes_p)
        self.tra_dq = dist_neg_bins(self.off, self.tra_p, self.tra_q, self.coords, self.dd, self.dist_num)

    def shard(self, lo=0, hi=None):
        """CsrTables of users [lo, hi) (offsets re-based); len_max stays the dataset-wide maximum, as
        in the reference where every user is padded to the longest sequence of the whole file."""
        hi = self.n_user if hi is None else hi
        off = np.asarray(self.off, np.int64)
        a, b = off[lo], off[hi]
        return CsrTables(off=(off[lo:hi + 1] - a).astype(np.int32), p=self.tra_p[a:b], q=self.tra_q[a:b],
                         dp=self.tra_dp[a:b], dq=self.tra_dq[a:b], len_max=self.len_max,
                         tes_p=self.tes_p[lo:hi].reshape(-1, 1), tes_q=self.tes_q[lo:hi].reshape(-1, 1),
                         tes_mask=np.ones((hi - lo, 1), np.int32), tes_dp=self.tes_dp[lo:hi].reshape(-1, 1))

    def last_pois(self):
        return np.asarray(self.tra_p)[np.asarray(self.off, np.int64)[1:] - 1]

    def to_padded(self):
        """The reference's nested tables: (train, test, dist) argument triples of the model ctors."""
        lm = self.len_max
        tra_buys = csr_to_padded(self.off, self.tra_p, self.n_item, lm)
        tra_neg = csr_to_padded(self.off, self.tra_q, self.n_item, lm)
        tra_dist = csr_to_padded(self.off, self.tra_dp, self.dist_num, lm)
        tra_dneg = csr_to_padded(self.off, self.tra_dq, self.dist_num, lm)
        tra_mask = (np.arange(lm)[None, :] < self.lens[:, None]).astype(np.int32)
        tes_buys = self.tes_p.reshape(-1, 1).astype(np.int32)
        tes_neg = self.tes_q.reshape(-1, 1).astype(np.int32)
        tes_dist = self.tes_dp.reshape(-1, 1).astype(np.int32)
        tes_mask = np.ones((self.n_user, 1), np.int32)
        return dict(train=[tra_buys, tra_mask, tra_neg], test=[tes_buys, tes_mask, tes_neg],
                    dist=[tra_dist, tes_dist, tra_dneg])


SHAPES = {
    # name: (n_item, n_user, max_len, dim)   BASELINE.json configs / BASELINE.md section 3
    "tiny": (300, 64, 12, 16),
    "foursquare": (10_000, 5_000, 20, 64),
    "gowalla": (100_000, 50_000, 50, 128),
    # one GPU's slice of BASELINE.json configs[4] (10 M POIs / 1 M users over 8 GPUs, dim 256, fp16 table): all POIs, 1/8 of the users
    "x1": (10_000_000, 125_000, 50, 256),
}


def _local_transitions(rng, coords, w, raw, local, n_nbr):
    """Check-in sequences with a learnable next-POI signal: with probability `local` the next POI is drawn among the
    n_nbr nearest neighbours of the current one (weights = global popularity), otherwise from the global Zipf law.
    Real check-in data is dominated by short hops (the premise of Distance2Pre's distance-interval head); i.i.d. Zipf
    draws carry nothing a sequence model could learn beyond popularity."""
    from scipy.spatial import cKDTree
    n_item, n_user = len(coords), len(raw)
    xy = np.stack([coords[:, 0] * 111.19, coords[:, 1] * 111.19 * np.cos(coords[:, 0].mean() * DEG)], 1)      # km, locally flat
    nbr = cKDTree(xy).query(xy, k=n_nbr + 1)[1][:, 1:]                                   # (n_item, n_nbr), self dropped
    cw = np.cumsum(w[nbr], axis=1); cw /= cw[:, -1:]
    cdf = np.cumsum(w / w.sum())
    lmax = int(raw.max())
    seq = np.empty((n_user, lmax), np.int64)
    seq[:, 0] = np.minimum(np.searchsorted(cdf, rng.random(n_user)), n_item - 1)
    for t in range(1, lmax):
        cur = seq[:, t - 1]
        loc = nbr[cur, np.minimum((cw[cur] < rng.random(n_user)[:, None]).sum(axis=1), n_nbr - 1)]
        glob = np.minimum(np.searchsorted(cdf, rng.random(n_user)), n_item - 1)
        seq[:, t] = np.where(rng.random(n_user) < local, loc, glob)
    return seq[np.arange(lmax)[None, :] < raw[:, None]]                                   # flat, user-major


def make_synthetic(n_user, n_item, max_len, seed, dd=200, ud_km=40, min_len=4, box_km=40.0, zipf=1.0, local=0.0, n_nbr=32):
    """Synthetic Foursquare/Gowalla-shaped data: lognormal sequence lengths clipped to
    [min_len, max_len] (+1 held-out check-in), Zipf POI popularity, POIs uniform in a ~box_km square.
    local = 0: every check-in is an independent Zipf draw (round-1 generator; nothing but popularity to learn);
    local > 0: that fraction of the transitions goes to one of the n_nbr nearest POIs of the current one."""
    rng = np.random.default_rng(seed)
    dist_num = int(ud_km * 1000 / dd)                    # prog_bpr_gru_spatial.py:81
    mu, sigma = np.log(max(max_len / 3.0, min_len)), 0.6
    lens = np.clip(np.rint(rng.lognormal(mu, sigma, n_user)), min_len, max_len).astype(np.int64)
    raw = lens + 1                                        # + the held-out last check-in (split = -1)
    w = 1.0 / np.power(np.arange(1, n_item + 1, dtype=np.float64), zipf)
    cdf = np.cumsum(w / w.sum())
    perm = rng.permutation(n_item)
    if local <= 0.0:
        ranks = np.minimum(np.searchsorted(cdf, rng.random(int(raw.sum()))), n_item - 1)
        pois = perm[ranks].astype(np.int32)
    lat = 40.0 + rng.random(n_item) * (box_km / 111.19)
    lon = -74.0 + rng.random(n_item) * (box_km / (111.19 * np.cos(40.0 * DEG)))
    coords = np.stack([lat, lon], 1)
    if local > 0.0:
        wp = np.empty(n_item); wp[perm] = w               # popularity weight of POI id i
        pois = _local_transitions(rng, coords, wp / wp.sum(), raw, float(local), int(n_nbr)).astype(np.int32)
    roff = np.zeros(n_user + 1, np.int64)
    np.cumsum(raw, out=roff[1:])
    rdist = dist_pos_bins(roff, pois, coords, dd, dist_num)
    is_last = np.zeros(len(pois), bool)
    is_last[roff[1:] - 1] = True
    off = np.zeros(n_user + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ds = PoiDataset(n_user=n_user, n_item=n_item, dist_num=dist_num, dd=float(dd), coords=coords,
                    off=off.astype(np.int32), tra_p=pois[~is_last], tra_dp=rdist[~is_last],
                    tes_p=pois[is_last], tes_dp=rdist[is_last])
    ds.resample_negatives(rng)
    return ds


def load_sequence_file(path, split=-1, dd=200, dist_num=200, seed=0, return_aliases=False):
    """The reference's `load_data` (public/Load_Data_by_length.py:45-112) on its own sequence file - the space-separated table the ETL writes
    (poidata/extract_whole_user_buys.py:81-90: columns check_times pois_different u_id u_pois u_times u_coordinates; `u_pois` = ids joined by
    '/', `u_coordinates` = 'lat,lon' pairs joined by '/') - straight into the CSR PoiDataset the generator returns.  Same rules:
      * train = upois[:split], held-out = upois[split] (split -1: test mode, -2: valid mode; :64-65);
      * distance bin of check-in i = cal_dis(check-in i, check-in i-1) from the PER-CHECK-IN coordinates, dist_num at i = 0 (:68-74);
      * a POI's coordinate in `coords` is the one of its LAST occurrence in file order (dict(zip(...)), :56);
      * n_item = number of distinct ids in the WHOLE file, held-out check-ins included (:57,98).
    Aliases: the reference numbers the POIs in the iteration order of a Python `set` of strings (:98-99) - arbitrary, and different from run to
    run under hash randomisation.  Here: order of first appearance in the file - a relabelling of the same data (tests/test_host_cpu.py checks
    equality with the reference's output modulo that relabelling).  Negatives are drawn as the driver does right after loading
    (prog_bpr_gru_spatial.py:88-91) from `seed`."""
    import pandas as pd
    tab = pd.read_csv(path, sep=" ")                                                      # :52
    seqs = [str(s).split("/") for s in tab["u_pois"]]
    cods = [[tuple(float(v) for v in c.split(",")) for c in str(s).split("/")] for s in tab["u_coordinates"]]
    alias, coord_of = {}, {}
    for upois, ucods in zip(seqs, cods):
        if len(upois) != len(ucods):
            raise ValueError("%s: a user with %d POIs and %d coordinates" % (path, len(upois), len(ucods)))
        if len(upois) < -split:
            raise IndexError("%s: a sequence of %d check-ins cannot be split at %d" % (path, len(upois), split))      # (the reference: IndexError at :65)
        for s_, c_ in zip(upois, ucods):
            if s_ not in alias:
                alias[s_] = len(alias)
            coord_of[s_] = c_
    n_user, n_item = len(seqs), len(alias)
    coords = np.empty((n_item, 2), np.float64)
    for s_, a_ in alias.items():
        coords[a_] = coord_of[s_]
    ids = [np.fromiter((alias[s_] for s_ in upois), np.int32, count=len(upois)) for upois in seqs]
    dist = []
    for ucods in cods:                                                                    # :68-74
        c = np.asarray(ucods, np.float64)
        d = np.full(len(c), dist_num, np.int64)
        if len(c) > 1:
            d[1:] = cal_dis_vec(c[1:, 0], c[1:, 1], c[:-1, 0], c[:-1, 1], dd, dist_num)
        dist.append(d.astype(np.int32))
    lens = np.array([len(x[:split]) for x in ids], np.int64)
    off = np.zeros(n_user + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ds = PoiDataset(n_user=n_user, n_item=n_item, dist_num=int(dist_num), dd=float(dd), coords=coords, off=off.astype(np.int32),
                    tra_p=np.concatenate([x[:split] for x in ids]).astype(np.int32), tra_dp=np.concatenate([d[:split] for d in dist]).astype(np.int32),
                    tes_p=np.array([x[split] for x in ids], np.int32), tes_dp=np.array([d[split] for d in dist], np.int32))
    ds.resample_negatives(np.random.default_rng(seed))
    return (ds, alias) if return_aliases else ds


def write_sequence_file(path, seqs, coords, user_ids=None):
    """Write check-in sequences in the ETL's format (poidata/extract_whole_user_buys.py:81-90) - the inverse of load_sequence_file, for tests and
    for handing synthetic data to the reference driver.  seqs: list of POI-id lists; coords: (n_item, 2) or a list of per-check-in lists."""
    import pandas as pd
    rows = []
    for k, s in enumerate(seqs):
        cc = coords[k] if isinstance(coords, list) else [coords[i] for i in s]
        rows.append((len(s), "%0.2f" % (1.0 * len(set(s)) / len(s)), user_ids[k] if user_ids is not None else k, "/".join(str(i) for i in s),
                     "/".join(str(t) for t in range(len(s))), "/".join("%r,%r" % (float(c[0]), float(c[1])) for c in cc)))
    cols = ["check_times", "pois_different", "u_id", "u_pois", "u_times", "u_coordinates"]
    pd.DataFrame(rows, columns=cols).to_csv(path, sep=" ", index=False, columns=cols)


def shard_users(n_user, world_size, rank, lens=None):
    """Contiguous user shard [lo, hi) of rank `rank`; with `lens`, boundaries balance the number of
    check-ins (GRU steps) rather than the number of users."""
    if lens is None:
        per = (n_user + world_size - 1) // world_size
        lo = min(rank * per, n_user)
        return lo, min(lo + per, n_user)
    c = np.concatenate(([0], np.cumsum(np.asarray(lens, np.int64))))
    tot = c[-1]
    bounds = [int(np.searchsorted(c, tot * r / world_size, side="left")) for r in range(world_size)] + [n_user]
    bounds[0] = 0
    for i in range(1, len(bounds)):
        bounds[i] = max(bounds[i], bounds[i - 1])
    return bounds[rank], bounds[rank + 1]


# ---- PRME (public/Load_Data_prme.py) ----------------------------------------------------------------------------------------------
PRME_R = 6378.137                    # Load_Data_prme.py:25


def prme_cal_dis(lat1, lon1, lat2, lon2):
    """public/Load_Data_prme.py:24-35, vectorised in the same float64 operation order (rad(x) = x * pi / 180, sin^2 of the halves)."""
    rad = lambda x: np.multiply(np.asarray(x, np.float64), np.pi) / 180.0
    rl1, rl2 = rad(lat1), rad(lat2)
    a = rl1 - rl2
    b = rad(lon1) - rad(lon2)
    s = 2 * np.arcsin(np.sqrt(np.power(np.sin(a / 2), 2) + np.cos(rl1) * np.cos(rl2) * np.power(np.sin(b / 2), 2)))
    return s * PRME_R


@dataclasses.dataclass
class PrmeDataset:
    """The tables prog_prme.py's Params builds (load_data + fun_data_pois_masks + the two negative draws), train side CSR-packed."""
    n_user: int
    n_item: int
    coords: np.ndarray          # (n_item + 1, 2) float64 lat, lon; row n_item = (0, 0) (`location`)
    off: np.ndarray             # (n_user + 1,) int32 train offsets
    tra_p: np.ndarray           # flat int32 train POIs
    tra_d: np.ndarray           # flat float64 km from the previous check-in (0 at a sequence's first check-in)
    tra_gap: np.ndarray         # flat int32 minutes since the previous check-in (0 at the first)
    tes_p: np.ndarray           # (n_user, len_tes) int32, padded with n_item
    tes_mask: np.ndarray        # (n_user, len_tes) int32
    tra_q: np.ndarray = None    # flat int32 train negatives (fun_random_neg_masks_tra)
    tes_q: np.ndarray = None    # (n_user, len_tes) test negatives (fun_random_neg_masks_tes), n_item on padding

    @property
    def lens(self):
        return np.diff(np.asarray(self.off, np.int64))

    def resample_negatives(self, rng):
        """prog_prme.py:179-182: train negatives outside the user's train list, test negatives outside train and test lists."""
        self.tra_q = random_neg_tra(rng, self.n_item, self.off, self.tra_p)
        m = np.asarray(self.tes_mask).astype(bool)
        tes_off = np.zeros(self.n_user + 1, np.int64)
        np.cumsum(m.sum(axis=1), out=tes_off[1:])
        flat = np.asarray(self.tes_p)[m]
        q = np.full(self.tes_p.shape, self.n_item, np.int32)
        q[m] = random_neg_tes(rng, self.n_item, self.off, self.tra_p, tes_off, flat)
        self.tes_q = q

    def last_pois(self):
        return np.asarray(self.tra_p)[np.asarray(self.off, np.int64)[1:] - 1]


def _prme_from_lists(seqs, times, cods, split, seed, where="input"):
    """Shared body of load_prme_sequence_file / make_prme_synthetic: per-user lists of raw POI keys, float times (minutes) and (lat, lon)."""
    s0, s1 = float(split[0]), float(split[1])
    alias, coord_of = {}, {}
    for upois, ucods in zip(seqs, cods):
        for s_, c_ in zip(upois, ucods):
            coord_of[s_] = c_                                             # :55-56, the last occurrence in the whole file
    tra, tes, tra_d, tra_g = [], [], [], []
    for upois, ut, ucods in zip(seqs, times, cods):
        le = len(upois)
        if not (len(ut) == len(ucods) == le):
            raise ValueError("%s: a user with %d POIs, %d times and %d coordinates" % (where, le, len(ut), len(ucods)))
        i1, i2 = int(le * s0), int(le * s1)                               # :66-68
        t = np.asarray(ut, np.float64)
        gap = np.zeros(le, np.float64)
        gap[1:] = t[1:] - t[:-1]
        if np.any(gap != np.round(gap)) or np.any(np.abs(gap) >= 2 ** 31):
            raise ValueError("%s: check-in time gaps must be whole minutes (the reference's gap is a Theano iscalar)" % where)
        c = np.asarray(ucods, np.float64).reshape(-1, 2)
        dist = np.zeros(le, np.float64)
        if le > 1:
            dist[1:] = prme_cal_dis(c[1:, 0], c[1:, 1], c[:-1, 0], c[:-1, 1])      # :73-79
        tra.append(upois[:i1]); tes.append(upois[i1:i2])
        tra_d.append(dist[:i1]); tra_g.append(gap[:i1].astype(np.int32))
    for utra, utes in zip(tra, tes):                                      # :102-105: numbering over the kept check-ins
        for s_ in list(utra) + list(utes):
            if s_ not in alias:
                alias[s_] = len(alias)
    dropped = [s_ for s_ in coord_of if s_ not in alias]
    if dropped:                                                           # the reference: KeyError at cordi_new[aliases_dict[i]]
        raise KeyError("%s: POI(s) %s occur only in the check-ins the split %s drops" % (where, dropped[:8], list(split)))
    n_user, n_item = len(seqs), len(alias)
    coords = np.zeros((n_item + 1, 2), np.float64)
    for s_, a_ in alias.items():
        coords[a_] = coord_of[s_]
    lens = np.array([len(x) for x in tra], np.int64)
    off = np.zeros(n_user + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    tl = np.array([len(x) for x in tes], np.int64)
    lt = int(tl.max()) if n_user else 0
    tes_p = np.full((n_user, lt), n_item, np.int32)
    for k, x in enumerate(tes):
        tes_p[k, :len(x)] = [alias[s_] for s_ in x]
    tes_mask = (np.arange(lt)[None, :] < tl[:, None]).astype(np.int32)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if len(xs) and off[-1] else np.zeros(0, dt)
    ds = PrmeDataset(n_user=n_user, n_item=n_item, coords=coords, off=off.astype(np.int32),
                     tra_p=cat([np.fromiter((alias[s_] for s_ in x), np.int32, count=len(x)) for x in tra], np.int32),
                     tra_d=cat(tra_d, np.float64), tra_gap=cat(tra_g, np.int32), tes_p=tes_p, tes_mask=tes_mask)
    ds.resample_negatives(np.random.default_rng(seed))
    return ds, alias


def load_prme_sequence_file(path, split=(0.8, 1.0), seed=0, return_aliases=False):
    """The reference's PRME loading (public/Load_Data_prme.py:38-120 load_data, fun_data_pois_masks, fun_random_neg_masks_tra / _tes as
    prog_prme.py:67-77 calls them) on the ETL's sequence file, into a PrmeDataset:
      * fractional split: train = pois[0:int(le*s0)], test = pois[int(le*s0):int(le*s1)] (test mode (0.8, 1.0), valid mode (0.6, 0.8));
      * gap[j] = t[j] - t[j-1] in minutes (must be whole: the reference's Theano iscalar) and dist[j] = cal_dis(c[j], c[j-1]) from the
        per-check-in coordinates, both 0 at j = 0;
      * n_item counts the distinct POIs of the kept check-ins; a POI seen only in the dropped tail raises KeyError, as the reference does;
      * a POI's coordinate is the one of its last occurrence in the whole file; coords gets a pad row n_item = (0, 0).
    Aliases: order of first appearance among the kept check-ins (train lists, then test lists, user by user) instead of the reference's
    set() iteration order - a relabelling of the same data.  Negatives are drawn from `seed` with the rules of poi_sample_negatives."""
    import pandas as pd
    tab = pd.read_csv(path, sep=" ")
    seqs = [str(s).split("/") for s in tab["u_pois"]]
    times = [[float(v) for v in str(s).split("/")] for s in tab["u_times"]]
    cods = [[tuple(float(v) for v in c.split(",")) for c in str(s).split("/")] for s in tab["u_coordinates"]]
    ds, alias = _prme_from_lists(seqs, times, cods, split, seed, where=str(path))
    return (ds, alias) if return_aliases else ds


def make_prme_synthetic(n_user, n_item, max_len, seed, far_frac=0.3, threshold=360, split=(0.8, 1.0), **kw):
    """make_synthetic's check-ins (lengths, popularity, optional locality `local=`) with check-in times whose gaps exceed `threshold`
    minutes with probability far_frac (else uniform in [1, threshold]), split and numbered as load_prme_sequence_file does."""
    base = make_synthetic(n_user, n_item, max_len, seed, **kw)
    rng = np.random.default_rng(seed + 1)
    off = np.asarray(base.off, np.int64)
    seqs, times, cods = [], [], []
    for u in range(n_user):
        s = np.concatenate([base.tra_p[off[u]:off[u + 1]], base.tes_p[u:u + 1]])
        g = np.where(rng.random(len(s)) < far_frac, rng.integers(threshold + 1, 10 * threshold, len(s)), rng.integers(1, threshold + 1, len(s)))
        g[0] = 0
        seqs.append(s.tolist()); times.append(np.cumsum(g).astype(np.float64).tolist()); cods.append([tuple(base.coords[i]) for i in s])
    return _prme_from_lists(seqs, times, cods, split, seed, where="make_prme_synthetic")[0]


# ---- GeoIE (public/Load_Data_GeoIE.py) --------------------------------------------------------------------------------------------
# The data are load_sequence_file's / make_synthetic's PoiDataset: the same split (train = upois[:split], held-out upois[split]), the same
# coordinates (a POI's last occurrence in the file) and the same negatives rule (fun_random_neg_masks_tra) as Load_Data_GeoIE.load_data.
def geoie_cal_dis(lat1, lon1, lat2, lon2):
    """cal_dis of Load_Data_GeoIE.py:28-42, vectorised in its float64 operation order (km)."""
    lat1, lon1, lat2, lon2 = (np.asarray(v, np.float64) for v in (lat1, lon1, lat2, lon2))
    a = (lat1 - lat2) * DEG
    b = (lon1 - lon2) * DEG
    c = (1.0 - np.cos(a)) / 2 + np.cos(lat1 * DEG) * np.cos(lat2 * DEG) * (1.0 - np.cos(b)) / 2
    return EARTH_D * np.arcsin(np.sqrt(c))


def geoie_pair_distances(coords, off, p, q, users=None):
    """fun_compute_dist_neg (Load_Data_GeoIE.py:143-156) without its zero padding, in poi_geoie_pair_distances' packed order: for each user
    of `users` (default all, in order) and each row i = 0 .. L-2, the float32 distances of p_0 .. p_i to p_{i+1} (dp) and to q_{i+1} (dq).
    Returns (dp, dq, pair offsets per user (len(users) + 1, int64), rows per user)."""
    xy = np.asarray(coords, np.float64)
    off = np.asarray(off, np.int64)
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    users = np.arange(len(off) - 1) if users is None else np.asarray(users, np.int64)
    rows = np.maximum(off[users + 1] - off[users] - 1, 0)
    poff = np.zeros(len(users) + 1, np.int64)
    np.cumsum(rows * (rows + 1) // 2, out=poff[1:])
    dp, dq = np.empty(int(poff[-1]), np.float32), np.empty(int(poff[-1]), np.float32)
    for k, u in enumerate(users):
        R = int(rows[k])
        if R == 0:
            continue
        s = p[off[u]:off[u + 1]]
        ii, jj = np.tril_indices(R)
        src, tp, tq = xy[s[jj]], xy[s[ii + 1]], xy[q[off[u] + ii + 1]]
        dp[poff[k]:poff[k + 1]] = geoie_cal_dis(src[:, 0], src[:, 1], tp[:, 0], tp[:, 1])
        dq[poff[k]:poff[k + 1]] = geoie_cal_dis(src[:, 0], src[:, 1], tq[:, 0], tq[:, 1])
    return dp, dq, poff, rows


# ---- POI2Vec (public/Load_Data_Poi2vec.py) ----------------------------------------------------------------------------------------
def poi2vec_region_tree(coords, theta):
    """The binary region tree of Load_Data_Poi2vec.py:152-247 (Treenode.build / route / overlap) over POI coordinates (n_item, 2) lat, lon,
    and the per-POI route tables of preprocess (:96-125).  Root box = (min lat, max lat, max lon, min lon); a node halves its longer side
    (latitude when strictly longer, else longitude) while that side > 2 theta, else it is a leaf.  Node ids follow the constructor order:
    root 0; a splitting node's children take the next two ids, then the left subtree is built before the right one.  Every level is built
    at once here (all nodes of a level have the same size, so the tree is perfect: ValueError if the arithmetic says otherwise, or if the
    box has an empty side), each node with the reference's own expressions for its bounds.
    Returns a dict: n_node, n_leaf, depth, routes (n_item + 1, 4, depth) int32 [leaf, .., root], lrs (same shape, int8: 1 at the leaf, then
    +1 / -1 for the left (lower latitude / upper longitude) / right child taken at each ancestor), probs (n_item + 1, 4) float32, rid
    (n_item + 1, 4) int32 = the leaf's left-to-right index (its ancestor at level l is node_ids[l][rid >> (depth - 1 - l)]), node_ids (list
    per level) and leaf_box (n_leaf, 4) left, right, up, down; row n_item is the pad row: routes[0], lrs[0], probs 0 (:128-130)."""
    xy = np.asarray(coords, np.float64).reshape(-1, 2)
    theta = float(theta)
    if not theta > 0 or len(xy) == 0:
        raise ValueError("poi2vec_region_tree: theta must be > 0 and coords non-empty")
    L, R, U, Dn = (np.array([v]) for v in (xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].max(), xy[:, 1].min()))
    if not (R[0] > L[0] and U[0] > Dn[0]):
        raise ValueError("poi2vec_region_tree: the bounding box of the coordinates has an empty side")
    levels = []
    while True:
        lat_split = (R - L) > (U - Dn)                                     # :171
        split = np.where(lat_split, (R - L) > 2 * theta, (U - Dn) > 2 * theta)
        if split.any() != split.all() or (split.all() and lat_split.any() != lat_split.all()):
            raise ValueError("poi2vec_region_tree: the nodes of level %d do not split alike (the tree is not perfect)" % len(levels))
        levels.append(dict(L=L, R=R, U=U, D=Dn, lat=bool(lat_split[0]) if split[0] else None))
        if not split[0]:
            break
        if len(levels) > 30:
            raise ValueError("poi2vec_region_tree: more than 2^30 leaves")
        n = len(L)
        nl, nr, nu, nd = (np.empty(2 * n) for _ in range(4))
        if lat_split[0]:                                                   # :174-176
            nl[0::2], nr[0::2], nl[1::2], nr[1::2] = L, (L + R) / 2, (R + L) / 2, R
            nu[0::2] = nu[1::2] = U; nd[0::2] = nd[1::2] = Dn
        else:                                                              # :184-186
            nl[0::2] = nl[1::2] = L; nr[0::2] = nr[1::2] = R
            nu[0::2], nd[0::2], nu[1::2], nd[1::2] = U, (U + Dn) / 2, (U + Dn) / 2, Dn
        L, R, U, Dn = nl, nr, nu, nd
    depth = len(levels)
    # numbering: a node with h levels below it and child counter c has children c, c + 1; its left child's counter is c + 2, its right
    # child's c + 2 + (2^h - 2) (the left subtree below the left child holds 2^h - 2 nodes)
    ids, cs = np.array([0], np.int64), np.array([1], np.int64)
    node_ids = [ids]
    for lv in range(depth - 1):
        h = depth - 1 - lv
        nid, ncs = np.empty(2 * len(ids), np.int64), np.empty(2 * len(ids), np.int64)
        nid[0::2], nid[1::2] = cs, cs + 1
        ncs[0::2], ncs[1::2] = cs + 2, cs + (1 << h)
        ids, cs = nid, ncs
        node_ids.append(ids)
    n_leaf = 1 << (depth - 1)
    n_node = 2 * n_leaf - 1
    # routes of the 4 corners of every POI (:99-112)
    n_item = len(xy)
    lat, lon = xy[:, 0], xy[:, 1]
    cl = np.stack([lat - 0.5 * theta, lat - 0.5 * theta, lat + 0.5 * theta, lat + 0.5 * theta], 1)
    co = np.stack([lon - 0.5 * theta, lon + 0.5 * theta, lon - 0.5 * theta, lon + 0.5 * theta], 1)
    k = np.zeros((n_item, 4), np.int64)
    for lv in range(depth - 1):
        ch = levels[lv + 1]
        if levels[lv]["lat"]:
            right = ch["R"][2 * k] < cl                                    # :213 left_child.right < latitude
        else:
            right = ch["D"][2 * k] > co                                    # :222 left_child.down > longitude
        k = 2 * k + right
    routes = np.empty((n_item + 1, 4, depth), np.int32)
    lrs = np.ones((n_item + 1, 4, depth), np.int8)
    for d in range(depth):
        routes[:n_item, :, d] = node_ids[depth - 1 - d][k >> d]
        if d >= 1:
            lrs[:n_item, :, d] = 1 - 2 * ((k >> (d - 1)) & 1)
    lf = levels[-1]
    left = np.maximum(lat[:, None] - 0.5 * theta, lf["L"][k])              # :161-166
    right = np.minimum(lat[:, None] + 0.5 * theta, lf["R"][k])
    up = np.minimum(lon[:, None] + 0.5 * theta, lf["U"][k])
    down = np.maximum(lon[:, None] - 0.5 * theta, lf["D"][k])
    area = (right - left) * (up - down)
    for r in range(1, 4):                                                  # :108-111: a route seen at an earlier corner counts once
        seen = np.zeros(n_item, bool)
        for r0 in range(r):
            seen |= k[:, r0] == k[:, r]
        area[seen, r] = 0
    probs = np.zeros((n_item + 1, 4), np.float32)
    probs[:n_item] = area / area.sum(axis=1, keepdims=True)
    rid = np.empty((n_item + 1, 4), np.int32)
    rid[:n_item] = k
    routes[n_item], lrs[n_item], rid[n_item] = routes[0], lrs[0], rid[0]
    return dict(n_node=int(n_node), n_leaf=int(n_leaf), depth=int(depth), routes=routes, lrs=lrs, probs=probs, rid=rid,
                node_ids=[a.astype(np.int32) for a in node_ids],
                leaf_box=np.stack([lf["L"], lf["R"], lf["U"], lf["D"]], 1), theta=theta)


@dataclasses.dataclass
class Poi2vecDataset:
    """What Load_Data_Poi2vec.preprocess / load_data / fun_data_masks hand to prog_poi2vec.py, contexts as CSR of CSR instead of the table
    padded to the longest context: user u's train positions are off[u] .. off[u+1]-1 of tra_t (targets); position x's context POIs are
    tra_c[tra_coff[x] .. tra_coff[x+1]-1]; the same on the test side."""
    n_user: int
    n_item: int
    n_node: int
    depth: int
    coords: np.ndarray          # (n_item, 2) float64 lat, lon
    off: np.ndarray             # (n_user + 1,) int32
    tra_t: np.ndarray           # flat int32 train targets
    tra_coff: np.ndarray        # (n_pos + 1,) int32
    tra_c: np.ndarray           # flat int32 train context POIs
    tes_off: np.ndarray
    tes_t: np.ndarray
    tes_coff: np.ndarray
    tes_c: np.ndarray
    routes: np.ndarray          # (n_item + 1, 4, depth) int32
    lrs: np.ndarray             # (n_item + 1, 4, depth) int8
    probs: np.ndarray           # (n_item + 1, 4) float32
    rid: np.ndarray             # (n_item + 1, 4) int32 left-to-right leaf index of each route
    theta: float = 0.1

    @property
    def lens(self):
        return np.diff(np.asarray(self.off, np.int64))

    @property
    def len_max(self):
        return int(self.lens.max()) if self.n_user else 0

    def tes_padded(self):
        """(tes_target_masks, tes_masks) of fun_data_masks (Load_Data_Poi2vec.py:133-139): targets padded with n_item."""
        tl = np.diff(np.asarray(self.tes_off, np.int64))
        lt = int(tl.max()) if self.n_user else 0
        mask = (np.arange(lt)[None, :] < tl[:, None]).astype(np.int32)
        p = np.full((self.n_user, lt), self.n_item, np.int32)
        p[mask.astype(bool)] = self.tes_t
        return p, mask


def poi2vec_contexts(times, time_threshold):
    """Load_Data_Poi2vec.py:56-69 for one user: for check-in j the earlier check-ins k = j-1, j-2, .. while t_j - t_k < time_threshold
    (stopping at the first that fails).  Returns the list of index lists (nearest first; only the multiset matters: contexts are summed)."""
    out = []
    for j in range(len(times)):
        ctx = []
        for k in range(j - 1, -1, -1):
            if times[j] - times[k] < time_threshold:
                ctx.append(k)
            else:
                break
        out.append(ctx)
    return out


def poi2vec_next_context(pois, times, now, time_threshold):
    """The loader's context rule (poi2vec_contexts, Load_Data_Poi2vec.py:56-69) applied to a QUERY at time `now` behind a history of
    check-ins `pois` at `times`: the trailing check-ins k = L-1, L-2, .. while now - t_k < time_threshold, stopping at the first that
    fails.  Returns their POI ids (nearest first) as an int64 array - what OboPoi2vec.score_new / recommend_new / rank_new take as one
    row of contexts=.  Host only."""
    pois, times = np.asarray(pois, np.int64).reshape(-1), np.asarray(times).reshape(-1)
    if len(pois) != len(times):
        raise ValueError("poi2vec_next_context: %d POIs and %d times" % (len(pois), len(times)))
    out = []
    for k in range(len(pois) - 1, -1, -1):
        if now - times[k] < time_threshold:
            out.append(int(pois[k]))
        else:
            break
    return np.asarray(out, np.int64)


def _poi2vec_from_lists(seqs, times, cods, split, time_threshold, region_threshold, where="input"):
    s1 = float(split[1])
    alias, coord_of = {}, {}
    for upois, ucods in zip(seqs, cods):
        for s_, c_ in zip(upois, ucods):
            if s_ not in alias:
                alias[s_] = len(alias)                                     # every POI of the file (:45, :81-82)
            coord_of[s_] = c_                                              # :43-44: the last occurrence in the file
    n_user, n_item = len(seqs), len(alias)
    coords = np.zeros((n_item, 2), np.float64)
    for s_, a_ in alias.items():
        coords[a_] = coord_of[s_]
    sides = {"tra": ([0], [], [0], []), "tes": ([0], [], [0], [])}
    for upois, ut in zip(seqs, times):
        le = len(upois)
        if len(ut) != le:
            raise ValueError("%s: a user with %d POIs and %d times" % (where, le, len(ut)))
        split1, split2 = int(le * s1 - 1), int(le * s1)                    # :56
        ids = [alias[s_] for s_ in upois]
        ctx = poi2vec_contexts(ut, time_threshold)
        for name, idx in (("tra", list(range(le))[0:split1]), ("tes", list(range(le))[split1:split2])):
            off, t, coff, c = sides[name]
            for j in idx:
                t.append(ids[j])
                c.extend(ids[k] for k in ctx[j])
                coff.append(len(c))
            off.append(len(t))
    tree = poi2vec_region_tree(coords, region_threshold)
    i32 = lambda v: np.asarray(v, np.int32)
    ds = Poi2vecDataset(n_user=n_user, n_item=n_item, n_node=tree["n_node"], depth=tree["depth"], coords=coords,
                        off=i32(sides["tra"][0]), tra_t=i32(sides["tra"][1]), tra_coff=i32(sides["tra"][2]), tra_c=i32(sides["tra"][3]),
                        tes_off=i32(sides["tes"][0]), tes_t=i32(sides["tes"][1]), tes_coff=i32(sides["tes"][2]), tes_c=i32(sides["tes"][3]),
                        routes=tree["routes"], lrs=tree["lrs"], probs=tree["probs"], rid=tree["rid"], theta=float(region_threshold))
    return ds, alias


def load_poi2vec_sequence_file(path, split=(0.8, 1.0), time_threshold=360, region_threshold=0.1, return_aliases=False):
    """Load_Data_Poi2vec.preprocess (:35-131) on the ETL's sequence file, into a Poi2vecDataset:
      * split1 = int(le * split[1] - 1), split2 = int(le * split[1]); train targets [0:split1], test targets [split1:split2] (split[0] is
        unused, as in the reference);
      * n_item counts every POI of the file; a POI's coordinate is the one of its last occurrence;
      * contexts: poi2vec_contexts on the integer check-in times; the tree and the route tables: poi2vec_region_tree.
    Aliases: order of first appearance in the file instead of the reference's set() iteration order - a relabelling of the same data."""
    import pandas as pd
    tab = pd.read_csv(path, sep=" ")
    seqs = [str(s).split("/") for s in tab["u_pois"]]
    times = [[int(v) for v in str(s).split("/")] for s in tab["u_times"]]
    cods = [[tuple(float(v) for v in c.split(",")) for c in str(s).split("/")] for s in tab["u_coordinates"]]
    ds, alias = _poi2vec_from_lists(seqs, times, cods, split, time_threshold, region_threshold, where=str(path))
    return (ds, alias) if return_aliases else ds


def make_poi2vec_synthetic(n_user, n_item, max_len, seed, far_frac=0.3, time_threshold=360, region_threshold=0.1, split=(0.8, 1.0), **kw):
    """make_prme_synthetic's check-ins and times (make_synthetic's lengths, popularity and optional locality `local=`; gaps above
    time_threshold minutes with probability far_frac), split and numbered as load_poi2vec_sequence_file does."""
    base = make_synthetic(n_user, n_item, max_len, seed, **kw)
    rng = np.random.default_rng(seed + 1)
    off = np.asarray(base.off, np.int64)
    seqs, times, cods = [], [], []
    for u in range(n_user):
        s = np.concatenate([base.tra_p[off[u]:off[u + 1]], base.tes_p[u:u + 1]])
        g = np.where(rng.random(len(s)) < far_frac, rng.integers(time_threshold + 1, 10 * time_threshold, len(s)),
                     rng.integers(1, time_threshold + 1, len(s)))
        g[0] = 0
        seqs.append(s.tolist()); times.append(np.cumsum(g).astype(np.int64).tolist()); cods.append([tuple(base.coords[i]) for i in s])
    return _poi2vec_from_lists(seqs, times, cods, split, time_threshold, region_threshold, where="make_poi2vec_synthetic")[0]


# ---- VBPR (public/BPR.py:245-335) ----------------------------------------------------------------------------------------------------
def synthetic_features(n_item, n_img, seed, scale=None):
    """(n_item + 1, n_img) float32 item features shaped like the post-ReLU CNN activations the reference's VBPR was written for (nothing in
    the reference loads a feature file): non-negative, about half of the entries zero, a few latent "styles" shared between items, row
    n_item the zero pad row.  scale multiplies the rows (None: unit scale, entries ~ |N(0, 1)|; 1 / sqrt(n_img) keeps ei . d of order 1)."""
    rng = np.random.default_rng(seed)
    n_style = max(2, min(16, n_item))
    styles = rng.standard_normal((n_style, n_img))
    mix = rng.dirichlet(np.full(n_style, 0.3), n_item)
    x = mix @ styles + 0.7 * rng.standard_normal((n_item, n_img))
    x = np.maximum(x, 0.0)
    if scale is not None:
        x = x * float(scale)
    out = np.zeros((n_item + 1, n_img), np.float32)
    out[:n_item] = x
    return out


# ---- filtered recommendation: POI attributes and pass bitmaps (include/poi_hip.h, poi_filter_build) ---------------------------------
def synthetic_attributes(n_item, n_cat, seed):
    """(categories (n_item) int32 in [0, n_cat), flags (n_item) uint32) for tests and benchmarks - nothing in the reference carries
    attributes.  Category sizes are very unequal (Zipf over a shuffled category order: a few categories hold most POIs, many hold a
    handful or none); flag bit 0 is set on about half of the POIs ("open now"), bit 1 on a tenth ("wheelchair access"), bits 2-3 hold a
    price tier 0 .. 3, bit 4 is set on about one POI in a hundred."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_cat + 1) ** 1.2
    cats = rng.permutation(n_cat)[rng.choice(n_cat, n_item, p=w / w.sum())].astype(np.int32)
    flags = ((rng.random(n_item) < 0.5).astype(np.uint32) | ((rng.random(n_item) < 0.1).astype(np.uint32) << 1)
             | (rng.integers(0, 4, n_item).astype(np.uint32) << 2) | ((rng.random(n_item) < 0.01).astype(np.uint32) << 4))
    return cats, flags.astype(np.uint32)


def pack_pass_bits(masks, ldw=None):
    """Boolean pass masks (P, n_item) (or (n_item): one predicate) -> the (P, ldw) uint32 bitmap the filtered top-K entries read: POI j
    is bit j & 31 of word j >> 5; the bits at j >= n_item are 0.  ldw defaults to ceil(n_item / 32).  numpy in, numpy out; a torch
    tensor in, a torch tensor (int32 storage of the same bits, on the tensor's device) out."""
    try:
        import torch
    except ImportError:      # pragma: no cover - torch is a hard dependency of the package, numpy callers do not need it here
        torch = None
    if torch is not None and isinstance(masks, torch.Tensor):
        m = masks.reshape(1, -1) if masks.dim() == 1 else masks
        P, N = m.shape
        W = (N + 31) // 32
        ldw = W if ldw is None else int(ldw)
        if ldw < W:
            raise ValueError("ldw must be >= ceil(n_item / 32) = %d (got %d)" % (W, ldw))
        b = torch.zeros((P, ldw * 32), dtype=torch.int64, device=m.device)
        b[:, :N] = m != 0
        sh = torch.arange(32, dtype=torch.int64, device=m.device)
        words = (b.view(P, ldw, 32) << sh).sum(dim=2)                                   # < 2^32, exact in int64
        return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)   # the same 32 bits
    m = np.asarray(masks)
    m = m.reshape(1, -1) if m.ndim == 1 else m
    P, N = m.shape
    W = (N + 31) // 32
    ldw = W if ldw is None else int(ldw)
    if ldw < W:
        raise ValueError("ldw must be >= ceil(n_item / 32) = %d (got %d)" % (W, ldw))
    b = np.zeros((P, ldw * 32), np.uint8)
    b[:, :N] = m != 0
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view("<u4").reshape(P, ldw)


def grid_labels(coords, cell_km):
    """Grid cells as labels for the capped top-K (models.poi_labels): coords (n_item, 2) lat, lon in degrees -> (labels (n_item) int32,
    n_label, centres (n_label, 2) float64).  Cells are equal-angle: cell_km kilometres of latitude (EARTH_D pi / 360 km per degree) by
    the same length of longitude at the table's MEAN latitude (the step is divided by its cosine), indexed by floor(lat / step) and
    floor(lon / step) - a cell never straddles the equator or the 0 degree meridian.  The occupied cells are numbered 0 .. n_label - 1 in
    the order of their first POI by ascending id; centres holds every cell's mid point.  Host numpy."""
    xy = np.asarray(coords.cpu().numpy() if hasattr(coords, "cpu") else coords, np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or len(xy) == 0:
        raise ValueError("coords must be (n_item >= 1, 2) lat, lon (got %s)" % (xy.shape,))
    if not float(cell_km) > 0.0:
        raise ValueError("cell_km must be > 0 (got %r)" % (cell_km,))
    km_per_deg = EARTH_D * np.pi / 360.0
    dlat = float(cell_km) / km_per_deg
    dlon = dlat / max(np.cos(xy[:, 0].mean() * DEG), 1e-6)
    cell = np.stack([np.floor(xy[:, 0] / dlat), np.floor(xy[:, 1] / dlon)], axis=1).astype(np.int64)
    _, first, inv = np.unique(cell, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                   # unique() sorts by cell: renumber by first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    labels = rank[np.asarray(inv).reshape(-1)].astype(np.int32)
    centres = (cell[first[order]] + 0.5) * np.array([dlat, dlon])
    return labels, int(len(order)), centres
