"""The score rows of tests/test_gpu_select.py, built on the host: tests/test_select_cpu.py checks under the oracle alone
(tests/select_oracle.py) that they contain what they claim, the GPU tests feed them to poi_topk_select.  float32 matrices, row r of a
fixture holding pattern PATTERNS[r % len(PATTERNS)]."""
import functools

import numpy as np

from tests import select_oracle as SO

# (rows, n_item): below / at / above a 32-row tile, several tiles, more rows than "select_split_max"; tables shorter than any k, one that
# is no multiple of anything, and 5000 ids - enough for k = 4096 and for 64 slices
SHAPES = {"one": (1, 5), "short": (31, 13), "odd": (33, 1037), "tile": (32, 3000), "big": (70, 5000), "many": (300, 1037)}
KS = (1, 20, 64, 65, 100, 1000, 1024, 1025, 4096)
PATTERNS = ("plateau", "eight", "cluster", "ascending", "descending", "special", "dead", "sparse", "normal", "eight_signed")
TIE_PATTERNS = ("plateau", "eight", "eight_signed")
ULP1 = float(2.0 ** -23)                            # the spacing of float32 in [1, 2)


def ks_of(n_item):
    return [k for k in KS if k <= min(n_item, SO.K_MAX)]


def pattern_row(name, n_item, rng):
    N = n_item
    if name == "plateau":                            # every score equal: the lowest ids win
        return np.full(N, 0.25, np.float32)
    if name == "eight":                              # 8 values: every tie group is spread over the whole id range (it straddles every slice)
        return rng.integers(-3, 5, N).astype(np.float32)
    if name == "eight_signed":                       # ... with both zeros among them
        v = rng.integers(-3, 5, N).astype(np.float32)
        v[(v == 0) & (rng.random(N) < 0.5)] = -0.0
        return v
    if name == "cluster":                            # 1 + i 2^-23, the top 1024 of them inside one block of 1024 mantissa steps: only the
        i = 8192 - N + rng.permutation(N)            # last digit pass (the low 10 bits) separates them
        return (1.0 + i * ULP1).astype(np.float32)
    if name == "ascending":
        return np.arange(N, dtype=np.float32)
    if name == "descending":
        return (N - np.arange(N)).astype(np.float32)
    if name == "special":                            # mixed signs with +-0.0, denormals, +-inf and NaN
        v = rng.normal(size=N).astype(np.float32)
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, np.nan, -np.nan, 3.4e38, -3.4e38], np.float32)
        hit = rng.random(N) < 0.3
        v[hit] = pool[rng.integers(0, len(pool), hit.sum())]
        return v
    if name == "dead":                               # nothing selectable
        return np.where(rng.random(N) < 0.5, np.float32(np.nan), np.float32(-np.inf)).astype(np.float32)
    if name == "sparse":                             # fewer selectable entries than any k > 7
        v = np.where(rng.random(N) < 0.5, np.float32(np.nan), np.float32(-np.inf)).astype(np.float32)
        j = rng.choice(N, min(7, N), replace=False)
        v[j] = rng.normal(size=len(j)).astype(np.float32)
        return v
    assert name == "normal"
    return rng.normal(size=N).astype(np.float32)


def pattern_of(r):
    return PATTERNS[r % len(PATTERNS)]


@functools.lru_cache(maxsize=None)
def fixture(shape):
    """dict(sc (n, n_item) float32, ex (off, ids) int32 CSR, name): the score rows and the exclusion lists of one shape.  Lists by
    row: empty, the row's ten best ids, random, and - on every eighth row - everything."""
    n, N = SHAPES[shape]
    rng = np.random.default_rng(1000 + 17 * n + N)
    sc = np.stack([pattern_row(pattern_of(r), N, rng) for r in range(n)])
    top, _, _, _ = SO.select(sc, min(10, N))
    lists = []
    for r in range(n):
        kind = (r // len(PATTERNS) + r) % 4
        if r % 8 == 7:
            lists.append(np.arange(N))
        elif kind == 0:
            lists.append(np.zeros(0, np.int64))
        elif kind == 1:
            lists.append(np.sort(top[r][top[r] >= 0]))
        else:
            lists.append(np.sort(rng.choice(N, rng.integers(0, min(60, N) + 1), replace=False)))
    return dict(name=shape, sc=sc, ex=SO.csr(lists))


@functools.lru_cache(maxsize=None)
def expected(shape, with_lists):
    """The oracle's lists of a fixture at the largest k it allows: (ids, scores, counts).  The list of a smaller k is its first k
    columns - the result is sorted best first, so a shorter list is a prefix of a longer one."""
    F = fixture(shape)
    ex = F["ex"] if with_lists else (None, None)
    ids, val, cnt, bad = SO.select(F["sc"], min(F["sc"].shape[1], SO.K_MAX), ex[0], ex[1])
    assert bad == 0
    return ids, val, cnt


def padded(sc, extra=3, fill=1e30):
    """The matrix with `extra` more columns per row (ld > n_item) that hold a large finite value: a kernel that reads them selects them."""
    out = np.full((sc.shape[0], sc.shape[1] + extra), fill, np.float32)
    out[:, :sc.shape[1]] = sc
    return out
