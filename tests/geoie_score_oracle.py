"""Float64 numpy restatement of GeoIE's TRAINED score rule (include/poi_hip.h, poi_geoie_score_all_geo) from
float32-rounded tables, with the distance and power-law conventions of tests/geoie_oracle.py:

    S(l) = tu . z[l] + (1 / L) sum_{k in distinct(history), ascending} m_k (g[k] . h[l]) f(max(f32(cal_dis(k, l)), d_min)),  f(d) = a d^b

and its absolute mass M(l) = |tu| . |z[l]| + (1 / L) sum_k m_k (|g[k]| . |h[l]|) |f|, the yardstick of a float32 kernel's error.
A pair at d_eff = 0 contributes 0 when b > 0 and makes S(l) NaN when b <= 0; an empty history scores tu . z[l] alone."""
import numpy as np

from poi_amd.data import geoie_cal_dis, make_synthetic
from tests.geoie_oracle import _f, init_tables


def compact(history):
    """history -> (distinct ids ascending, multiplicities)."""
    ks, m = np.unique(np.asarray(history, np.int64), return_counts=True)
    return ks, m


def scores_geo(P, history, coords, d_min, tu=None):
    """(S, M), each (n_item,) float64.  P: dict of float64 tables g / h / z (n_item + 1, D) and scalars a / b (geoie_oracle.round_f32)."""
    xy = np.asarray(coords, np.float64)
    n_item = P["g"].shape[0] - 1
    g, h, z = P["g"], P["h"][:n_item], P["z"][:n_item]
    a, b = float(P["a"]), float(P["b"])
    history = np.asarray(history, np.int64)
    L = len(history)
    if tu is None:
        S, M = np.zeros(n_item), np.zeros(n_item)
    else:
        tu = np.asarray(tu, np.float64)
        S, M = z @ tu, np.abs(z) @ np.abs(tu)
    if L == 0:
        return S, M
    ks, mk = compact(history)
    acc, mass = np.zeros(n_item), np.zeros(n_item)
    nan = np.zeros(n_item, bool)
    every = np.ones(n_item, bool)
    for k, m in zip(ks, mk):
        d32 = geoie_cal_dis(xy[k, 0], xy[k, 1], xy[:, 0], xy[:, 1]).astype(np.float32)
        f, _, _, _ = _f(d32, a, b, d_min, every)                      # 0 where d_eff = 0
        if not b > 0:
            nan |= np.maximum(d32.astype(np.float64), d_min) == 0.0
        acc += m * (h @ g[k]) * f
        mass += m * (np.abs(h) @ np.abs(g[k])) * np.abs(f)
    S = S + acc / L
    M = M + mass / L
    S[nan] = np.nan
    return S, M


def scores_geo_literal(P, history, coords, d_min, tu=None):
    """The same rule as the double loop over OCCURRENCES (no compaction), one pair at a time: S only."""
    xy = np.asarray(coords, np.float64)
    n_item = P["g"].shape[0] - 1
    a, b = float(P["a"]), float(P["b"])
    history = np.asarray(history, np.int64)
    L = len(history)
    out = np.zeros(n_item)
    for l in range(n_item):
        s = float(np.dot(tu, P["z"][l])) if tu is not None else 0.0
        geo = 0.0
        for pj in history:
            d = float(np.float32(geoie_cal_dis(xy[pj, 0], xy[pj, 1], xy[l, 0], xy[l, 1])))
            d = max(d, d_min)
            if d == 0.0:
                if not b > 0:
                    geo = np.nan
                continue
            geo += float(np.dot(P["g"][pj], P["h"][l])) * a * d ** b
        out[l] = s + (geo / L if L else 0.0)
    return out


def planted_problem(n_user=600, n_item=800, max_len=40, seed=13, dim=20):
    """The problem of the GPU signal test: test_train_geoie_learns' data (a user's next POI is drawn near the previous ones) with planted
    tables - g, h uniform(0, 0.5) so that g.h > 0, f decreasing with the distance (a = 0.3, b = -0.3)."""
    ds = make_synthetic(n_user, n_item, max_len, seed, local=0.9, n_nbr=8)
    rng = np.random.default_rng(seed)
    init = init_tables(rng, ds.n_user, ds.n_item, dim)
    init["g"], init["h"] = np.abs(init["g"]), np.abs(init["h"])
    init["a"], init["b"] = 0.3, -0.3
    return ds, init
