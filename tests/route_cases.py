"""The problems of tests/test_gpu_route.py, built on the host: tests/test_route_cpu.py checks on the CPU that the oracle alone decides
at least 75 % of the slots of every fixture with clear gaps (tests/route_oracle.clear), the GPU tests build the models from them.
Problems and parameters come from geo_problem / spatial_init / gru_init of tests/test_gpu_session.py and from
tests/session_cells_oracle.py; a slot's history is its user's training row (4 .. 12 check-ins), exclusion = the last POI + own path."""
import functools

import numpy as np

from tests import route_oracle as RO
from tests import session_cells_oracle as S
from tests.test_gpu_session import geo_problem, gru_init, seqs_of, spatial_init

CLEAR_MIN = 0.75

# name -> (kind, n_dist, dim, n_item, beam, steps, slots)
SHAPES = {
    "d20":       (11, 20, 50, 4, 6, 24),
    "d20x40":    (11, 20, 50, 4, 6, 40),
    "d64":       (11, 64, 100, 4, 6, 24),
    "d128":      (200, 128, 300, 4, 4, 24),
    "d128b2":    (200, 128, 300, 2, 6, 24),
    "d16x144":   (11, 16, 70, 4, 8, 144),          # 576 hypothesis rows: the advance takes the session tile path
    "d256":      (11, 256, 100, 2, 3, 6),
    "small":     (11, 20, 27, 3, 4, 12),           # n_item < 32: one partial item tile
    "one":       (11, 20, 50, 4, 6, 1),            # n = 1
    "b8":        (200, 128, 300, 8, 4, 24),
    "t16":       (200, 128, 300, 2, 16, 24),
}
FIXTURES = [(kind, name) for name in SHAPES for kind in ("spatial", "plain")] + [("lstm", "d20"), ("rnn", "d64")]


@functools.lru_cache(maxsize=None)
def problem(kind, name):
    """dict(T, P, kind, beam, steps, hist (the slots' histories))."""
    n_dist, dim, n_item, beam, steps, slots = SHAPES[name]
    T = geo_problem(7 + dim + n_dist, n_user=slots, n_item=n_item, n_dist=n_dist, dim=dim, len_min=4, len_max=12)
    if kind == "spatial":
        P = spatial_init(dim, T)
    elif kind == "plain":
        P = gru_init(dim, T)
    else:
        P = S.cell_params(dim, T, kind)
    return dict(T=T, P=P, kind=kind, beam=beam, steps=steps, hist=[tuple(int(v) for v in q) for q in seqs_of(T)])


@functools.lru_cache(maxsize=None)
def solve(kind, name):
    """The oracle's routes of every slot of a fixture (exclude = the last POI) and which slots are clear:
    dict(scorer, paths (n, beam, steps), total (n, beam), steplp, clear (n) bool, max_abs)."""
    C = problem(kind, name)
    sc = RO.Scorer(kind, C["P"], C["T"])
    res = [RO.beam_search(sc, h, C["beam"], C["steps"], exclude=(h[-1],)) for h in C["hist"]]
    ok = np.array([RO.clear(r["gaps"], sc.max_abs) for r in res])
    return dict(scorer=sc, paths=np.array([r["paths"] for r in res]), total=np.array([r["total"] for r in res]),
                steplp=np.array([r["steplp"] for r in res]), clear=ok, max_abs=sc.max_abs)
