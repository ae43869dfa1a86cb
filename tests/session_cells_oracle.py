"""Oracle side of the Lstm / Rnn / CA-RNN session tests (tests/test_session_cells_cpu.py, tests/test_gpu_session_cells.py): parameters,
per-prefix float64 states from tests/cells_oracle.py and oracle/poi_oracle.py, and the condition that keeps the CA-RNN comparison from
running blind.

CA-RNN's literal predict step is h = sigmoid(M x + rowsum(wd[d]) + sum(h_prev)).  With the reference's uniform(-0.5, 0.5) init the
scalar sum(h_prev) ~ D / 2 pushes every unit to exactly 1.0 after two steps, and a comparison of such states sees nothing.  So the
tests draw wd[b] as uniform(-0.5, 0.5) - (b % 3) / 2 per element: the row sums of two bins in three then cancel sum(h_prev) often
enough that a good share of the states keeps entries inside (0.05, 0.95) - `informative` counts them, on the oracle alone."""
import numpy as np

from oracle import poi_oracle as O
from tests import cells_oracle as C
from tests.gpu_util import round_f32

INFORMATIVE_MIN = 0.15      # share of the (user, prefix) states that must be informative


def cell_params(seed, T, cell):
    """The reference's uniform(-0.5, 0.5) init with a non-zero bias, rounded to float32."""
    rng = np.random.default_rng(seed + 3000)
    P = C.init_params(rng, T["n_item"], T["dim"], cell)
    P["bi"] = rng.uniform(-0.2, 0.2, P["bi"].shape)
    return round_f32(P)


def carnn_params(seed, T, shifted=True):
    rng = np.random.default_rng(seed + 4000)
    P = O.init_carnn_params(rng, T["n_item"], T["n_dist"], T["dim"])
    if shifted:
        P["wd"] = P["wd"] - ((np.arange(T["n_dist"] + 1) % 3) / 2.0)[:, None, None]
    return round_f32(P)


def cell_prefix_states(P, cell, seq):
    """-> (h (L, D), c (L, D)): the state after each check-in of one sequence, from h0 = c0 = 0."""
    D = P["lt"].shape[1]
    h, c = np.zeros(D), np.zeros(D)
    hs, cs = [], []
    for j in seq:
        h, c, _ = C.cell_step(P, cell, P["lt"][j], h, c)
        hs.append(h); cs.append(c)
    return np.array(hs), np.array(cs)


def carnn_prefix_states(P, seq, bins):
    """-> h (L, D): oracle.carnn_predict on every prefix p[:t + 1] of one sequence."""
    return np.array([O.carnn_predict(P, P["lt"], P["wd"], [list(seq[:t + 1])], [list(bins[:t + 1])], [np.ones(t + 1, int)])[0]
                     for t in range(len(seq))])


def informative(states):
    """bool per state (rows of an (n, D) array): half or more of its entries lie in (0.05, 0.95)."""
    s = np.asarray(states)
    return ((s > 0.05) & (s < 0.95)).mean(axis=1) >= 0.5
