"""Integer model of the fixed-point scheme that csrc/te_xfwd.hip documents in its header, in numpy integers (CPU only).

An operand row is scaled by a power of two to |Q| <= 2^38, Q = rint(v 2^(38 - e)), and cut into five signed base-256 digits;
the product of two rows is 2^(e_a + e_b - 12) x sum_w 256^-w acc_w with acc_w = sum_{i + j = w} d_i . e_j summed exactly in int32,
w <= 4 (te_gemmx<64|128>, te_rec_fwdx) or w <= 6 (te_gemmx<256>); the classes are merged as x_merge<K> / x_merge7 merge them,
int32 wrap-around included.  h and r * h are cut at the fixed scale 2^38 (e_a = 0).

This model is NOT the judge of anything: the judge of the GPU tests is the float64 oracle.  It serves to
  * assert that planted rows have the digits they claim (tests/xfwd_cases.py, tests/test_xfwd_cases_cpu.py),
  * compute the accumulator magnitudes the planted rows reach (the head-room table of DESIGN.md section 2),
  * supply mutants - the scheme with one plausible defect each - which the regimes must expose at the GPU tests' bar.

MUTANTS
  exp_pow2   the row exponent of a row whose largest entry is an exact power of two, 2^k, is taken as k - 1: one below the smallest
             exponent that still holds the row (the kernel takes k + 1: |Q| = 2^37; k would do: |Q| = 2^38, leading digit 64; at k - 1
             |Q| = 2^39 leaves the five digits and wraps modulo 2^40).
  wrap23     te_gemmx<256> with the K <= 128 merge: classes 0 .. 4 only, (a2 << 8) + a3 in int32.
  drop34     digits 3 and 4 of both operands dropped (every product, the chain's included).
  zero_row   the exponent of an all-zero row is not clamped at float32's smallest: it comes out of log2(0) = -inf, the scale
             2^(38 - e) is inf and 0 x inf = NaN in every product of the row.
"""
import numpy as np

XS = 5
XQB = 8 * XS - 2
MUTANTS = ("exp_pow2", "wrap23", "drop34", "zero_row")
_BIAS = 0x8080808080
_M40 = (1 << 40) - 1


def row_exponent(rows32, mutant=None):
    """x_exponent of every row's largest |entry|: e with |m| < 2^e; zero and subnormal rows: -126.  rows32: (n, K) float32."""
    rows32 = np.ascontiguousarray(rows32, np.float32)
    m = np.abs(rows32).max(axis=1).astype(np.float32)
    bits = m.view(np.uint32).astype(np.int64)
    e = ((bits >> 23) & 255) - 126
    if mutant == "exp_pow2":
        pow2 = ((bits & 0x7FFFFF) == 0) & (((bits >> 23) & 255) > 0)
        e = np.where(pow2, e - 2, e)
    return e


def quantize(rows, e):
    """Q = rint(v 2^(38 - e)) as int64 (round half to even, as the 1.5 x 2^52 trick of x_digits rounds)."""
    return np.rint(np.ldexp(np.asarray(rows, np.float64), (XQB - np.asarray(e))[:, None])).astype(np.int64)


def digits(Q):
    """Five signed base-256 digits d_0 (leading) .. d_4 of Q, Q = sum_s d_s 256^(4 - s), d_s in [-128, 127]: the bytes of
    (Q + 0x8080808080) mod 2^40, each less 128 - the bias trick of x_digits, wrap-around included."""
    u = (np.asarray(Q, np.int64) + _BIAS) & _M40
    return np.stack([((u >> (8 * (XS - 1 - s))) & 255) - 128 for s in range(XS)], axis=-1)


def undigits(d):
    return sum(np.asarray(d, np.int64)[..., s] << (8 * (XS - 1 - s)) for s in range(XS))


def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def class_sums(DA, DB, wmax):
    """acc[w][r][n] = sum_{i + j = w} DA[r, :, i] . DB[n, :, j] (int64; |d e| <= 2^14 and K <= 256 terms: exact in float64 BLAS)."""
    n, N = DA.shape[0], DB.shape[0]
    acc = np.zeros((wmax + 1, n, N), np.int64)
    A = DA.astype(np.float64); B = DB.astype(np.float64)
    for i in range(XS):
        for j in range(XS):
            if i + j <= wmax:
                acc[i + j] += np.rint(A[:, :, i] @ B[:, :, j].T).astype(np.int64)
    return acc


class Stats:
    """Largest magnitudes met: `acc` any class accumulator, `m01` / `m23` the int32 merges, per site ("gemmx" / "chain")."""
    def __init__(self):
        self.v = {}

    def see(self, site, name, x):
        k = (site, name)
        self.v[k] = max(self.v.get(k, 0), int(np.abs(x).max()) if np.size(x) else 0)

    def get(self, site, name):
        return self.v.get((site, name), 0)


def merge(acc, wide, stats=None, site="gemmx"):
    """256 x sum_w acc_w 256^-w in float64: x_merge<K <= 128> (wide False: five classes, both int32 merges) or x_merge7 (wide True)."""
    a = [acc[w] for w in range(acc.shape[0])]
    m01x = (a[0] << 8) + a[1]
    if stats is not None:
        stats.see(site, "acc", acc); stats.see(site, "m01", m01x)
    m01 = wrap32(m01x).astype(np.float64)
    if not wide:
        m23x = (a[2] << 8) + a[3]
        if stats is not None:
            stats.see(site, "m23", m23x)
        m23 = wrap32(m23x).astype(np.float64)
        return (a[4].astype(np.float64) * 2.0 ** -8 + m23) * 2.0 ** -16 + m01
    t = a[6].astype(np.float64) * 2.0 ** -8 + a[5]
    for w in (4, 3, 2):
        t = t * 2.0 ** -8 + a[w]
    return t * 2.0 ** -8 + m01


def _operand(rows32, mutant):
    rows32 = np.ascontiguousarray(rows32, np.float32)
    e = row_exponent(rows32, mutant)
    d = digits(quantize(rows32, e))
    bad = np.zeros(len(e), bool)
    if mutant == "zero_row":
        bad = np.abs(rows32).max(axis=1) == 0
    if mutant == "drop34":
        d = d.copy(); d[..., 3:] = 0
    return d, e, bad


def product(A32, B32, mutant=None, stats=None):
    """te_gemmx: C[r][n] = A32[r] . B32[n] from the digit products (float64).  K = 256 keeps the classes 0 .. 6."""
    K = A32.shape[1]
    wide = K > 128 and mutant != "wrap23"
    DA, ea, bad_a = _operand(A32, mutant)
    DB, eb, bad_b = _operand(B32, mutant)
    v = merge(class_sums(DA, DB, 6 if wide else 4), wide, stats, "gemmx")
    out = np.ldexp(v, (ea[:, None] + eb[None, :] - 20))
    out[bad_a, :] = np.nan; out[:, bad_b] = np.nan
    return out


class ChainWeights:
    """The recurrent weights of one gate as te_xpack leaves them (digits + row exponents)."""
    def __init__(self, W32, mutant=None):
        self.d, self.e, self.bad = _operand(W32, mutant)
        self.mutant = mutant


def chain_product(state, W, stats=None):
    """te_rec_fwdx: state (n, K) in [-1, 1] cut at the fixed scale 2^38 (x_digits38) x weight rows -> (n, rows) float64."""
    Q = np.rint(np.ldexp(np.asarray(state, np.float64), XQB)).astype(np.int64)
    d = digits(Q)
    if W.mutant == "drop34":
        d = d.copy(); d[..., 3:] = 0
    v = merge(class_sums(d, W.d, 4), False, stats, "chain")
    out = np.ldexp(v, (W.e[None, :] - 20))
    out[:, W.bad] = np.nan
    return out


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(P, p_rows, d_rows, lens, arith="f64", mutant=None, stats=None):
    """Final hidden states (n, D) of the GRU forward recurrence from h_0 = 0 (the oracle's _gru_cell order of operations), batched over the
    sequences.  d_rows None: the plain GRU.  arith:
      "f64" / "ld"   plain float64 / np.longdouble arithmetic (the conditioning gate compares the two),
      "model"        the input product by product(), the recurrent products by chain_product() at dims <= 128 and in float64 at dim 256
                     (te_rec_fwdd multiplies in float64), the bin half of the input product and the gates in float64 (te_xztab)."""
    ft = np.longdouble if arith == "ld" else np.float64
    lt = np.asarray(P["lt"]); D = lt.shape[1]
    ui = np.asarray(P["ui"], ft); wh = np.asarray(P["wh"], ft); bi = np.asarray(P["bi"], ft)
    spatial = d_rows is not None
    p_rows = np.asarray(p_rows); lens = np.asarray(lens)
    n = len(lens)
    used = np.unique(np.concatenate([p_rows[k, :lens[k]] for k in range(n)]))
    pos = {int(r): i for i, r in enumerate(used)}
    Wi = ui[:, :, :D].reshape(3 * D, D)
    if arith == "model":
        G = product(lt[used].astype(np.float32), np.asarray(P["ui"])[:, :, :D].reshape(3 * D, D).astype(np.float32), mutant, stats)
        cw = [ChainWeights(np.asarray(P["wh"][g], np.float32), mutant) for g in range(3)] if D <= 128 else None
    else:
        G = np.asarray(lt[used], ft) @ Wi.T
        cw = None
    Z = bi.reshape(1, 3 * D)
    if spatial:
        Z = np.asarray(P["di"], ft) @ ui[:, :, D:].reshape(3 * D, D).T + Z
    h = np.zeros((n, D), ft)

    def rec(g, s):
        if cw is not None:
            return chain_product(s, cw[g], stats)
        return s @ wh[g].T

    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(int(lens.max())):
            on = np.nonzero(lens > t)[0]
            pre = G[[pos[int(p_rows[k, t])] for k in on]] + (Z[np.asarray(d_rows)[on, t]] if spatial else Z)
            hp = h[on]
            z = _sigmoid(pre[:, :D] + rec(0, hp))
            r = _sigmoid(pre[:, D:2 * D] + rec(1, hp))
            c = np.tanh(pre[:, 2 * D:] + rec(2, r * hp))
            h[on] = (1.0 - z) * hp + z * c
    return h


def rel_gap(a, b):
    """max |a - b| / max |b| (NaN counts as infinitely far)."""
    a = np.asarray(a, np.longdouble); b = np.asarray(b, np.longdouble)
    d = np.abs(a - b)
    if not np.isfinite(np.asarray(d, np.float64)).all():
        return float("inf")
    return float(d.max() / max(float(np.abs(b).max()), 1e-30))


# ------------------------------------------------------------------------------------------------
# the largest merges float32 rows can reach
# ------------------------------------------------------------------------------------------------
def f32_exact(Q):
    """Is the integer Q (|Q| <= 2^38) x 2^-38 a float32?  (24 significant bits.)"""
    Q = abs(int(Q))
    return Q == 0 or (Q >> max(Q.bit_length() - 24, 0)) << max(Q.bit_length() - 24, 0) == Q


def extreme_entries():
    """Candidate scaled integers Q of a float32 entry that is its row's largest, 2^37 <= |Q| <= 2^38: every choice of extreme digits
    d_0 in +-{62, 63, 64}, d_1, d_2 in {-128, 127}, d_3 in {-128, -64, 0, 64} that 24 significant bits can hold."""
    out = []
    for d0 in (-64, -63, -62, 62, 63, 64):
        for d1 in (-128, 127):
            for d2 in (-128, 127):
                for d3 in (-128, -64, 0, 64):
                    Q = (d0 << 32) + (d1 << 24) + (d2 << 16) + (d3 << 8)
                    if (1 << 37) <= abs(Q) <= (1 << 38) and f32_exact(Q):
                        out.append(Q)
    return out


def worst_pair():
    """The pair (Qa, Qb) of extreme_entries() whose per-k contribution to (a2 << 8) + a3 is largest in magnitude, and that contribution:
    a row of K such entries on both operands reaches K times it."""
    best = (0, 0, 0)
    E = extreme_entries()
    D = digits(np.array(E, np.int64))
    for ia, da in enumerate(D):
        for ib, db in enumerate(D):
            a2 = sum(int(da[i]) * int(db[2 - i]) for i in range(3))
            a3 = sum(int(da[i]) * int(db[3 - i]) for i in range(4))
            v = (a2 << 8) + a3
            if abs(v) > abs(best[2]):
                best = (E[ia], E[ib], v)
    return best
