"""Problems for the mini-batch Lstm / Rnn step (csrc/cells.hip) at the launch sizes where its kernels change what they do, shared by the
CPU twins (tests/test_cells_cpu.py) and the GPU tests (tests/test_gpu_cells_launch_sizes.py).  numpy only.

Unlike tests/gpu_util.toy_problem, positives and negatives are drawn from the WHOLE range [0, n_item): with many more POIs than
entries almost every POI row is touched by one or two sorted entries, so an entry the sort loses or credits to a neighbouring row is the
whole of that row's update and not a 1e-3 share of a hot row's.  On top of that
  * row 0, row n_item - 1 and the pad row n_item are named explicitly (the pad row as a real negative, next to its analytic touches);
  * about 5 % of the positives go to a few planted hot POIs, whose runs cross many 64-entry windows at the larger sizes.

The switches, mirrored here as pure functions of the launch so that every test can assert that its case crosses the one it is named for:
  sort_passes     launch_radix_sort's pass count (csrc/te_scatter.hip:353) for the key width launch_cell_step derives from n_item + 1
  position_rows   P, the launch's position rows; sort_entries = 2 P + 1 (cell_commit's grid is capped at 16384 of them);
                  windows = ceil((2 P + 1) / 64) (cell_rows / cell_span are capped at 8192 workgroups)
  chunk_rows      cell_chunk_rows(n, max_len): position rows per dense-gradient chunk (CELL_DENSE_CHUNKS = 64 chunks)
  rec_grid        cell_grid(n, 0): the persistent recurrent grid, CELL_GRID_MAX = 512"""
import numpy as np

PLAN_BLOCK = 256            # cell_plan_kernel scans the launch in blocks of 256 users
GRID_MAX = 512              # CELL_GRID_MAX
COMMIT_GRID_MAX = 16384     # launch_cell_step: cell_commit_kernel's grid cap, in sorted entries
WINDOW = 64                 # sorted entries per window of cell_rows_kernel / cell_span_kernel
WINDOW_GRID_MAX = 8192      # launch_cell_step: grid cap of cell_rows_kernel / cell_span_kernel, in windows
DENSE_CHUNKS = 64           # CELL_DENSE_CHUNKS


def sort_passes(n_item):
    """Passes of launch_radix_sort for a table of n_item POIs.  launch_cell_step (csrc/cells.hip) sorts keys of
    `bits` = the bit length of n_item + 1 (the sentinel, the largest key); csrc/te_scatter.hip:353 reads
    `npass = bits <= 9 ? 1 : bits <= 18 ? 2 : bits <= 27 ? 3 : 4`.  An odd pass count leaves the result in the second buffer pair
    (keys1 / vals1), an even one in the first."""
    bits = int(n_item + 1).bit_length()
    return 1 if bits <= 9 else 2 if bits <= 18 else 3 if bits <= 27 else 4


def chunk_rows(n, max_len):
    """cell_chunk_rows (csrc/cells.hip): ceil(n max_len / 64) rounded up to a multiple of 8, at least 8."""
    ch = -(-(n * max_len) // DENSE_CHUNKS)
    return max(8, (ch + 7) & ~7)


def rec_grid(n):
    return max(1, min(n, GRID_MAX))


def position_rows(case, idxs):
    return int(case["lens"][np.asarray(idxs)].sum())


def sort_entries(case, idxs):
    return 2 * position_rows(case, idxs) + 1


def windows(case, idxs):
    return -(-sort_entries(case, idxs) // WINDOW)


def pad_multiplicity(case, idxs):
    """The pad row's analytic touches: 2 (len_max - L) per user of the launch."""
    idxs = np.asarray(idxs)
    return int(2 * (case["len_max"] * len(idxs) - case["lens"][idxs].sum()))


def max_len(case):
    return int(case["lens"].max())


def problem(seed, n_user, n_item, len_max, lens, dim=8, hot_share=0.05, plant=(0, 1, 2), plant_pad=True):
    """Padded tables in the reference layout (tests/gpu_util.toy_problem's keys).  lens: one length per user, or (lo, hi) for uniform
    draws in [lo, hi] with user 0 at hi.  plant: three users that name row 0 (first positive), row n_item - 1 (last negative) and - with
    plant_pad - the pad row n_item (first negative)."""
    rng = np.random.default_rng(seed)
    if isinstance(lens, tuple):
        lo, hi = lens
        lens = rng.integers(lo, hi + 1, n_user)
        lens[0] = hi
    lens = np.asarray(lens, np.int64).copy()
    assert len(lens) == n_user and lens.min() >= 1 and lens.max() <= len_max
    M = (np.arange(len_max)[None, :] < lens[:, None]).astype(int)
    live = M > 0
    hot = np.unique(np.array([n_item // 3, n_item // 2, n_item - 2]))
    P = rng.integers(0, n_item, (n_user, len_max))
    P = np.where(rng.random((n_user, len_max)) < hot_share, hot[rng.integers(0, len(hot), (n_user, len_max))], P)
    Q = rng.integers(0, n_item, (n_user, len_max))
    P[plant[0], 0] = 0
    Q[plant[1], lens[plant[1]] - 1] = n_item - 1
    if plant_pad:
        Q[plant[2], 0] = n_item
    P, Q = np.where(live, P, n_item), np.where(live, Q, n_item)
    tes = lambda: rng.integers(0, n_item, (n_user, 1))
    return dict(train=[P, M, Q], test=[tes(), np.ones((n_user, 1), int), tes()], lens=lens, hot=hot, n_user=n_user, n_item=n_item,
                dim=dim, len_max=len_max)


def params(seed, n_item, dim, cell):
    """The reference's init range (tests/cells_oracle.init_params) with a non-zero bias, rounded to float32: the device tables are
    float32 and the oracle runs in float64 from exactly those values."""
    from tests import cells_oracle as C
    rng = np.random.default_rng(seed + 3000)
    P = C.init_params(rng, n_item, dim, cell)
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape)
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in P.items()}


def tables(case, idxs):
    """(p, q, mask) rows of the users idxs."""
    idxs = np.asarray(idxs)
    Pm, Mm, Qm = case["train"]
    return Pm[idxs], Qm[idxs], Mm[idxs]


# ---- the cases of tests/test_gpu_cells_launch_sizes.py ---------------------------------------------------------------------------------
A_N_ITEM = (510, 511, 262142, 262143)
A_PASSES = (1, 2, 2, 3)


def case_a(n_item, full):
    """Sort passes: 40 users, len_max 11; ragged (the pad row carries its analytic multiplicity) or every user at full length (slot
    2 P holds the sentinel n_item + 1 and the pad row must not move)."""
    return problem(100 + n_item % 1000 + full, 40, n_item, 11, [11] * 40 if full else (4, 11), plant_pad=not full)


B_SIZES = (255, 256, 257, 513, 769)
B_N_USER = 800


def case_b():
    """Plan blocks and the persistent grid: an 800-user model with 600 POIs, launches of b_users(n).  Lengths 8 .. 11 keep the pad
    row's multiplicity of the largest launch near 2000, where an off-by-one still shows (tests/test_cells_cpu.py)."""
    order = np.random.default_rng(71).permutation(B_N_USER)
    case = problem(70, B_N_USER, 600, 11, (8, 11), plant=tuple(order[:3]))
    Pm, Mm, Qm = case["train"]
    for u in order[[PLAN_BLOCK - 1, PLAN_BLOCK]]:             # length 1 on either side of the first block boundary of the plan scan
        Pm[u, 1:] = Qm[u, 1:] = 600
        Mm[u, 1:] = 0
        case["lens"][u] = 1
    case["order"] = order.astype(np.int32)
    return case


def b_users(case, n):
    return case["order"][:n]


def case_c1():
    """Commit cap: 513 users of 16 - 17 positions, 2 P + 1 > 16384."""
    return problem(81, 513, 600, 17, (16, 17))


def case_c2():
    """Sparse dense-gradient chunks: 64 users of length 1 - 2 and a 65th at 50 that no launch uses: P is about 100 against the
    bound n x max_len = 3200 the chunking is sized for."""
    lens = np.random.default_rng(82).integers(1, 3, 65)
    lens[0], lens[1], lens[64] = 1, 2, 50
    return problem(82, 65, 600, 50, lens)


D_N_USER, D_N_ITEM = 5300, 262143


def case_d(n_user=D_N_USER, dim=8):
    """Window cap: every user at 50 positions but the last one (49), three sort passes.  n_user = 5300 is the first multiple of 100
    whose 2 P + 1 entries need more than 8192 windows; smaller n_user give the reduced replica of the CPU sensitivity twins."""
    lens = np.full(n_user, 50)
    lens[-1] = 49
    return problem(90, n_user, D_N_ITEM, 50, lens, dim=dim)


E_DIMS = (4, 12, 100, 252)


def case_e(dim):
    return problem(300 + dim, 9, 70, 6, (2, 6), dim=dim)
