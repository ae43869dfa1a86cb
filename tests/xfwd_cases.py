"""Weight regimes beyond the reference's init range for the exact forward pass (csrc/te_xfwd.hip), and the launches that run them.
CPU only: shared by tests/test_xfwd_cases_cpu.py (conditioning gate, sharpness) and tests/test_gpu_xfwd_ranges.py (the GPU parity tests).

Every other test of the suite draws its weights from uniform(-0.5, 0.5): every row's largest entry lies in [0.25, 0.5) - one power-of-two
scale for every row of every operand -, no row is zero, no entry is a power of two, no row mixes magnitudes and no gate saturates.  A
regime here is a function (seed, dim, n_item, n_dist) -> P, float32-rounded, with the keys of gpu_util.spatial_params; the plain GRU
uses gru_subset(P)."""
from collections import namedtuple

import numpy as np

from oracle import poi_oracle as O
from tests import xfwd_model as M
from tests.gpu_util import round_f32, toy_problem


def _base(seed, dim, n_item, n_dist):
    rng = np.random.default_rng(seed + 1000)
    P = O.init_spatial_params(rng, n_item, n_dist, dim)
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape); P["bs"] = rng.uniform(-0.2, 0.2, P["bs"].shape)
    return P, rng


def gru_subset(P):
    d = P["lt"].shape[1]
    return dict(lt=P["lt"], ui=np.ascontiguousarray(P["ui"][:, :, :d]), wh=P["wh"], bi=P["bi"], h0=P["h0"])


def _pow2_rows(rng, rows, cols, klo, khi, span=None):
    """Rows whose largest |entry| is exactly 2^k (every third row: the float32 just below it), k drawn per row from klo .. khi, random
    sign, planted in one of the first `span` columns; every other entry is below 0.98 x 2^k."""
    k = rng.integers(klo, khi + 1, rows)
    out = rng.uniform(-0.98, 0.98, (rows, cols)) * 2.0 ** k[:, None]
    top = np.float32(2.0) ** k.astype(np.float32)
    below = np.nextafter(top, np.float32(0), dtype=np.float32)
    top = np.where(np.arange(rows) % 3 == 2, below, top).astype(np.float64)
    out[np.arange(rows), rng.integers(0, span or cols, rows)] = rng.choice([-1.0, 1.0], rows) * top
    return out


def pow2(seed, dim, n_item, n_dist):
    P, rng = _base(seed, dim, n_item, n_dist)
    P["lt"] = _pow2_rows(rng, n_item + 1, dim, -20, 1)
    P["di"] = _pow2_rows(rng, n_dist + 1, dim, -20, 1)
    P["ui"] = np.stack([_pow2_rows(rng, dim, 2 * dim, -6, 0, span=dim) for _ in range(3)])      # (the POI half carries the row's scale)
    P["wh"] = np.stack([_pow2_rows(rng, dim, dim, -6, 0) for _ in range(3)])
    return round_f32(P)


def wide(seed, dim, n_item, n_dist):
    """Every entry scaled by 2^(-8 j), j in 0 .. 3 drawn per entry: an entry populates the digits j .. j + 2 of its row only."""
    P, rng = _base(seed, dim, n_item, n_dist)
    for k in ("lt", "di", "ui", "wh"):
        P[k] = P[k] * 2.0 ** (-8.0 * rng.integers(0, 4, P[k].shape))
    return round_f32(P)


def extreme_digits(seed, dim, n_item, n_dist):
    """Rows of lt, ui[g][:, :dim] and wh[g] whose every entry is ONE float32 value with extreme leading digits (xfwd_model.extreme_entries:
    d_0 = +-62 .. 64, d_1, d_2 = 127 / -128, what 24 bits leave of d_3): equal signs along the whole row, on both operands, so every
    digit product of a class has the same sign and the int32 class sums and merges grow as far as float32 rows can push them.  Every
    fourth lt row and every fourth ui / wh row hold the pair xfwd_model.worst_pair() found.  The row scales are chosen so that the
    pre-activations stay O(1): the gates do not saturate and a wrong product is visible in the state."""
    P, rng = _base(seed, dim, n_item, n_dist)
    E = np.array(M.extreme_entries(), np.int64)
    qa, qb, _ = M.worst_pair()
    lg = int(np.log2(dim))

    def rows(n, q_lead, elo, ehi):
        q = rng.choice(E, n); q[::4] = q_lead
        e = rng.integers(elo, ehi + 1, n)
        return np.ldexp(q.astype(np.float64), e - M.XQB)[:, None]
    P["lt"] = np.repeat(rows(n_item + 1, qa, -1, 1), dim, axis=1)
    for g in range(3):
        P["ui"][g][:, :dim] = np.repeat(rows(dim, qb, -lg, 1 - lg), dim, axis=1)
        P["ui"][g][:, dim:] *= 0.5
        P["wh"][g] = np.repeat(rows(dim, qb, -lg, 1 - lg), dim, axis=1)
    return round_f32(P)


def zero_rows(seed, dim, n_item, n_dist):
    P, rng = _base(seed, dim, n_item, n_dist)
    P["lt"][n_item] = 0.0; P["lt"][1::2] = 0.0
    P["ui"][1][1::2] = 0.0
    P["wh"][0] = 0.0
    P["wh"][2][5] = 0.0
    P["di"][3] = 1e-40                       # (a float32 subnormal)
    P["bi"] = np.zeros_like(P["bi"])
    return round_f32(P)


def tiny(seed, dim, n_item, n_dist):
    P, rng = _base(seed, dim, n_item, n_dist)
    P["lt"] = P["lt"] * 1e-20; P["di"] = P["di"] * 1e-20; P["wh"] = P["wh"] * 1e-3
    return round_f32(P)


def huge(seed, dim, n_item, n_dist):
    """Every third POI row x 1e12: the gates saturate, h reaches +-1 exactly (Q = +-2^38 in the chain's digits)."""
    P, rng = _base(seed, dim, n_item, n_dist)
    P["lt"][::3] *= 1e12
    return round_f32(P)


def _trained(seed, dim, n_item, n_dist, gain):
    P, rng = _base(seed, dim, n_item, n_dist)
    lt = P["lt"] / np.linalg.norm(P["lt"], axis=1, keepdims=True)
    P["lt"] = lt * np.exp(rng.uniform(np.log(1e-3), np.log(30.0), (n_item + 1, 1)))
    P["ui"] = P["ui"] * gain; P["wh"] = P["wh"] * gain
    return round_f32(P)


def trained(seed, dim, n_item, n_dist):
    """POI row norms log-uniform over [1e-3, 30] (popular rows grown, the pad row decayed), ui and wh x 2: sequences of at most 12."""
    return _trained(seed, dim, n_item, n_dist, 2.0)


def trained4(seed, dim, n_item, n_dist):
    """trained with ui and wh x 4 (saturating gates): sequences of at most 6."""
    return _trained(seed, dim, n_item, n_dist, 4.0)


REGIMES = dict(pow2=pow2, wide=wide, extreme_digits=extreme_digits, zero_rows=zero_rows, tiny=tiny, huge=huge, trained=trained, trained4=trained4)


def pad_to(P, width):
    """P zero-padded to `width` hidden units (the device stores dim 20 as 64): the same forward map on the leading units."""
    d = P["lt"].shape[1]
    if d == width:
        return P
    out = dict(P)
    out["lt"] = np.pad(P["lt"], ((0, 0), (0, width - d)))
    out["wh"] = np.pad(P["wh"], ((0, 0), (0, width - d), (0, width - d)))
    out["bi"] = np.pad(P["bi"], ((0, 0), (0, width - d)))
    out["h0"] = np.zeros(width)
    if P["ui"].shape[2] == 2 * d:
        ui = np.zeros((3, width, 2 * width))
        ui[:, :d, :d] = P["ui"][:, :, :d]; ui[:, :d, width:width + d] = P["ui"][:, :, d:]
        out["ui"] = ui
        out["di"] = np.pad(P["di"], ((0, 0), (0, width - d)))
    else:
        out["ui"] = np.pad(P["ui"], ((0, 0), (0, width - d), (0, width - d)))
    return out


# ------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "regime dim n_seq len_max n_item n_dist spatial")


def case_id(c):
    return "%s-d%d-n%d-L%d-i%d-b%d%s" % (c.regime, c.dim, c.n_seq, c.len_max, c.n_item, c.n_dist, "" if c.spatial else "-gru")


def problem(c, seed=0):
    """toy_problem's padded tables, every user generated at full length and then cut: the lengths cycle through len_max, 1, 2, 12 and
    random ones, so a launch mixes the shortest sequences with the longest."""
    T = toy_problem(7000 + seed + c.dim + c.n_seq, n_user=c.n_seq, n_item=c.n_item, n_dist=c.n_dist, dim=c.dim, len_max=c.len_max,
                    min_len=c.len_max, hot=min(c.n_item, 300))
    rng = np.random.default_rng(7001 + seed + c.n_seq)
    lens = rng.integers(1, c.len_max + 1, c.n_seq)
    for u in range(c.n_seq):
        if u % 5 < 4:
            lens[u] = min((c.len_max, 1, 2, 12)[u % 5], c.len_max)
    for u, L in enumerate(lens):
        T["train"][0][u, L:] = c.n_item; T["train"][2][u, L:] = c.n_item
        T["dist"][0][u, L:] = c.n_dist; T["dist"][2][u, L:] = c.n_dist
        T["train"][1][u, L:] = 0
    T["lens"] = lens
    return T


def params(c, seed=0):
    P = REGIMES[c.regime](40 + seed + c.dim, c.dim, c.n_item, c.n_dist)
    return P if c.spatial else gru_subset(P)


def _shapes(regime, long_ok=True, dims=(64, 128, 256)):
    """The three standing shapes: dim 64 - 17 sequences, 11 bins, a 60-POI table (forward table); dim 128 - 40 sequences of up to 50
    positions where the regime's conditioning allows, 200 bins, 3000 POIs (per-step rows); dim 256 - 40 sequences, 200 bins, 60 POIs."""
    S = {64: (17, 12, 60, 11), 128: (40, 50 if long_ok else 12, 3000, 200), 256: (40, 12, 60, 200)}
    return [Case(regime, d, *S[d], True) for d in dims]


def _with(cases, **kw):
    return [c._replace(**kw) for c in cases]


PREDICT_CASES = (
    _shapes("pow2") + _shapes("wide") + _shapes("zero_rows") + _shapes("tiny") + _shapes("huge")
    + _shapes("trained", long_ok=False, dims=(64, 128)) + _with(_shapes("trained", dims=(256,)), len_max=10)      # (dim 256, 12 positions: the chain's own float64 gap passes 1e-11)
    + _with(_shapes("trained4", long_ok=False, dims=(64, 256)), len_max=6)
    + _with(_shapes("extreme_digits", long_ok=False), len_max=2) + _with(_shapes("extreme_digits", dims=(64, 128)), len_max=1)
    + [Case("pow2", 128, 1, 12, 60, 11, True), Case("zero_rows", 64, 1, 2, 3000, 200, True),      # one sequence
       Case("pow2", 20, 17, 12, 60, 11, True),                                                    # dim 20: stored zero-padded to 64
       Case("pow2", 128, 40, 12, 60, 11, False), Case("zero_rows", 64, 17, 12, 3000, 11, False),    # the plain GRU
       Case("extreme_digits", 128, 17, 2, 60, 11, False)])

STEP_CASES = (
    [Case(r, 64, 17, 12, 60, 11, True) for r in ("pow2", "wide", "zero_rows", "trained")]
    + [Case(r, 128, 40, 12, 3000, 200, True) for r in ("pow2", "wide", "zero_rows", "trained")]
    + [Case("pow2", 256, 17, 12, 60, 200, True), Case("zero_rows", 256, 17, 12, 60, 200, True), Case("trained", 256, 17, 10, 60, 200, True)]
    + [Case("pow2", 128, 1, 12, 60, 11, True), Case("trained", 64, 1, 12, 60, 200, True)])        # one sequence: the one-sequence path

# every (regime, dim, length) the GPU tests run: the conditioning gate of tests/test_xfwd_cases_cpu.py covers each
ALL_CASES = list(dict.fromkeys(PREDICT_CASES + STEP_CASES))
