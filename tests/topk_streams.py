"""Planted score rows for the streaming top-K kernels (score_topk.hip, score_filter.hip): numpy only.

Every value is a multiple of 2^-8 with magnitude below 2^10, so float32 and float64 hold the same numbers, sums with a distance term
that is a multiple of 2^-5 stay exact, and the oracle (oracle.poi_oracle.topk_desc on the same matrix) can be compared with ZERO
tolerance on ids and on score bits.  The families aim at what random scores never produce: exact ties at every rank, thresholds that
keep rising (candidate lists of 65 .. 80 entries), constant rows, a plateau at the cut that spans several item ranges, winners in the
first / last items of a ragged table, and values that differ only below half precision.

`list_model` restates one item range's candidate list (32-item tiles, insert when score > threshold, compaction to the K best when the
list exceeds 48 entries, capacity 80): tests/test_topk_streams_cpu.py uses it to show that the staircases reach the long-list states
from ANY range start, without reading kernel state.

A row that falls from tile to tile can never do that - after the first compaction (at exactly 64 entries: two tiles, everything beats
-inf) the threshold is the K-th best of the two highest tiles and nothing later passes.  `staircase_down` is that literal mirror image
and pins the opposite extreme (one compaction, then silence, ties against a bound that arrives at once); `staircase_up_mirrored` is the
mirror image INSIDE each tile (winners at the tile's end, falling within the tile), which keeps the long lists."""
import numpy as np

TILE = 32
LOW = -1000.0
PATTERN = (32, 32, 16, 32)
Q = 1.0 / 256.0          # the grid of every value


def _ntile(N):
    return (N + TILE - 1) // TILE


def staircase_up(N, mirrored=False, low=LOW):
    """a. Tile t holds m_t items at level 64 t + i (in units of 2^-8), m cycling through PATTERN; the rest sit at `low`."""
    row = np.full(N, float(low))
    for t in range(_ntile(N)):
        m = PATTERN[t % 4]
        for i in range(m):
            j = TILE * t + (TILE - 1 - i if mirrored else i)
            if j < N:
                row[j] = (64 * t + i) * Q
    return row


def staircase_up_mirrored(N, low=LOW):
    return staircase_up(N, mirrored=True, low=low)


def staircase_down(N, low=LOW):
    """b. The mirror image of family a: the levels fall from tile to tile and inside every tile."""
    nt = _ntile(N)
    row = np.full(N, float(low))
    for t in range(nt):
        m = PATTERN[t % 4]
        for i in range(m):
            j = TILE * t + i
            if j < N:
                row[j] = (64 * (nt - 1 - t) + (m - 1 - i)) * Q
    return row


def constant(N, value):
    """c."""
    return np.full(N, float(value))


def plateau(N, K, value):
    """d. K - 3 distinct high values at scattered positions, a plateau of equal values (>= 200 members from N = 2065 on) spread evenly
    over the whole row, everything else lower: the list ends with the three lowest-index plateau members."""
    j = np.arange(N)
    row = value - 1.0 - (j % 5) * 0.25
    stride = max(2, N // 210)
    row[j % stride == 3 % stride] = value
    n_high = max(0, min(K - 3, N // 4))
    for i in range(n_high):
        row[(i * N) // n_high + (5 * i) % max(1, N // n_high)] = value + 1.0 + ((37 * i) % 64) * Q
    return row


def plateau_late(N, K, value, first=250, every=2):
    """d'. As d, but the plateau starts late: its three lowest members sit at first, first + 10, first + 20 (tiles 7 and 8 of the first
    item range when ranges are nine tiles long - after that range's first refresh of the bounds other ranges published), and from
    first + 38 on every second (`every`-th) item is a member: a range that starts there sees K plateau members in its first two tiles and publishes
    the plateau as its K-th best while the first range has not yet met the members that belong on the list."""
    if N < first + 100:
        return plateau(N, K, value)
    j = np.arange(N)
    row = value - 1.0 - (j % 5) * 0.25
    row[[first, first + 10, first + 20]] = value
    row[first + 38::every] = value
    n_high = max(0, K - 3)
    for i in range(n_high):
        row[(i * N) // n_high + 1] = value + 1.0 + ((37 * i) % 64) * Q
    return row


def two_level(N):
    """e. Two values only: ties at every rank."""
    j = np.arange(N)
    return np.where((j * 7) % 5 < 2, 1.5, 0.75)


def mod7(N, step=0.25):
    """e. j mod 7 in quarter steps."""
    return (np.arange(N) % 7) * step


def edges(N):
    """f. Equal winners only in items 0 .. 2 and in the last three items; the rest cycles through three lower values."""
    j = np.arange(N)
    row = -1.0 - (j % 3) * 0.5
    row[:3] = 5.0
    row[max(N - 3, 0):] = 5.0
    return row


def half_planes(N):
    """g. About 20 significant bits, distinct over 101 neighbours, all within 1/2 of 512: IEEE half (spacing 1/2 there) collapses them
    to 512 or 512.5.  For the f16 filter only."""
    j = np.arange(N)
    return 512.0 + ((j * 37) % 101) * Q


def family_rows(N, K, with_g=False):
    """(names, (R, N) float64 matrix): one row per family member."""
    fams = [("a up", staircase_up(N)), ("a up, mirrored in the tile", staircase_up_mirrored(N)), ("b down", staircase_down(N)),
            ("c zero", constant(N, 0.0)), ("c 3.25", constant(N, 3.25)), ("d plateau 2.5", plateau(N, K, 2.5)), ("d plateau 0", plateau(N, K, 0.0)),
            ("d late plateau 0", plateau_late(N, K, 0.0)), ("d late plateau -4", plateau_late(N, K, -4.0)),
            ("e two levels", two_level(N)), ("e mod 7", mod7(N)), ("f edges", edges(N))]
    if with_g:
        fams.append(("g half planes", half_planes(N)))
    return [f[0] for f in fams], np.stack([f[1] for f in fams])


def half_planes_sparse(N):
    """g for lists the f16 filter can hold: every third item is 64 + k / 256, k < 16 - sixteen distinct float32 values that IEEE half
    (spacing 1/16 there) collapses to 64 or 64.0625 - and the rest sits far below, in five levels around 32."""
    j = np.arange(N)
    return np.where(j % 3 == 0, 64.0 + ((j * 37) % 16) * Q, 32.0 + (j % 5) * 0.25)


def filter_rows(N, K):
    """Rows for the two-stage path's OWN result (score_filter.hip: f16 filter, then score_rescore_kernel).  A user with more than 4096
    survivors hands the whole 32-user tile to the one-stage kernel, so no row here may keep that many items within the filter's error
    bound of its K-th best - about 2^-10 |item row|_2, i.e. ~0.15 with every magnitude at or below 64: no constant rows, no -1000, the
    dense plateau on every third item, mod 7 in half steps, and g on a third of the items.  (Constant rows and the -1000 staircases
    stay in family_rows, where they exercise the overflow fallback.)"""
    fams = [("a up", staircase_up(N, low=-4.0)), ("a up, mirrored in the tile", staircase_up_mirrored(N, low=-4.0)), ("b down", staircase_down(N, low=-4.0)),
            ("d plateau 2.5", plateau(N, K, 2.5)), ("d plateau 0", plateau(N, K, 0.0)),
            ("d late plateau 0", plateau_late(N, K, 0.0, every=3)), ("d late plateau -4", plateau_late(N, K, -4.0, every=3)),
            ("e two levels", two_level(N)), ("e mod 7", mod7(N, 0.5)), ("f edges", edges(N)), ("g sparse half planes", half_planes_sparse(N))]
    return [f[0] for f in fams], np.stack([f[1] for f in fams])


def is_exact(a):
    """Multiples of 2^-8 below 2^10 (float32 == float64 bit for bit)."""
    a = np.asarray(a, np.float64)
    return bool(np.all(np.abs(a) < 1024.0) and np.all(a * 256.0 == np.round(a * 256.0)) and np.array_equal(a.astype(np.float32).astype(np.float64), a))


def one_hot(S, n, dim, n_cls=None):
    """users (n, dim), items (N, dim) with users[u] . items[j] == S[u mod n_cls][j] exactly (n_cls = dim unless given; rows of S beyond
    its own are zero)."""
    S = np.asarray(S, np.float64)
    full = np.zeros((dim, S.shape[1]))
    full[:S.shape[0]] = S
    users = np.zeros((n, dim), np.float32)
    users[np.arange(n), np.arange(n) % (n_cls or dim)] = 1.0
    return users, np.ascontiguousarray(full.T.astype(np.float32)), full


def list_model(row, K, t0, nt, cap=80, trigger=48):
    """One item range's candidate list: tiles t0 .. t0 + nt - 1 of `row`.  Returns (lengths at which the list was compacted, final list
    of (score, index) best first)."""
    thr, lst, lens = -np.inf, [], []
    for t in range(t0, min(t0 + nt, _ntile(len(row)))):
        lst += [(s, j) for j, s in enumerate(row[TILE * t:TILE * (t + 1)], TILE * t) if s > thr]
        assert len(lst) <= cap, "the list overflows its %d slots" % cap
        if len(lst) > trigger:
            lens.append(len(lst))
            lst.sort(key=lambda e: (-e[0], e[1]))
            if len(lst) > K:
                lst = lst[:K]
                thr = lst[-1][0]
    lst.sort(key=lambda e: (-e[0], e[1]))
    return lens, lst[:K]


def expected_lists(S, K, topk_desc):
    """The contract of poi_topk / poi_score_topk*: descending score, ties by ascending index; an entry that is NaN or -inf is never
    selected, and a row with fewer than K selectable entries ends in -1 ids / -inf scores.  Returns (ids int32, scores float32)."""
    S = np.asarray(S, np.float64)
    X = np.where(np.isnan(S), -np.inf, S)
    idx = np.asarray(topk_desc(X, K))
    sc = np.take_along_axis(X, idx, axis=1)
    idx = np.where(sc > -np.inf, idx, -1)
    return idx.astype(np.int32), sc.astype(np.float32)
