"""CPU tests of the route recommendation's host side: the oracle against a brute force that enumerates every path, the declarations
(include/poi_hip.h, build.SOURCES), the host argument checks of Session.recommend_route, and the condition on the fixtures of
tests/test_gpu_route.py - in every fixture at least 75 % of the slots are decided with clear gaps under the oracle alone
(tests/route_oracle.clear), so that a float32 kernel must reproduce their routes exactly.  No GPU."""
import os
import re

import numpy as np
import pytest

import poi_amd
from poi_amd import models as M
from tests import route_cases as RC
from tests import route_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TableScorer:
    """A scorer over a made-up model: the scores of a state are a fixed function of the last two check-ins."""

    def __init__(self, n_item, seed):
        self.n_item = n_item
        self.tab = np.random.default_rng(seed).uniform(-2, 2, (n_item + 1, n_item + 1, n_item))
        self.max_abs = 2.0

    def scores(self, seq):
        a = seq[-1] if len(seq) > 0 else self.n_item
        b = seq[-2] if len(seq) > 1 else self.n_item
        return self.tab[a, b]


@pytest.mark.parametrize("revisit", [False, True])
def test_oracle_matches_a_brute_force(revisit):
    sc = TableScorer(7, 5)
    for hist, ex in (((3, 1), (1,)), ((), ()), ((0, 6, 2), (2, 4))):
        got = RO.beam_search(sc, hist, 2, 3, exclude=ex, revisit=revisit)
        kept, totals = RO.brute_force(sc, hist, 2, 3, exclude=ex, revisit=revisit)
        assert [tuple(p) for p in got["paths"]] == kept, (hist, got["paths"], kept)
        assert np.allclose(got["total"], totals, rtol=1e-13, atol=0)
        for k, p in enumerate(kept):
            lp, steps = RO.path_logp(sc, hist, p)
            assert abs(lp - got["total"][k]) <= 1e-12 and np.allclose(steps, got["steplp"][k], rtol=0, atol=1e-12)


def test_oracle_runs_out_of_candidates():
    sc = TableScorer(4, 6)
    got = RO.beam_search(sc, (0,), 3, 5, exclude=(0,))                 # 3 candidates, then 2, 1, 0
    assert (got["paths"][:, :3] >= 0).all() and (got["paths"][:, 3:] == -1).all() and np.isneginf(got["total"]).all()
    for p in got["paths"]:
        assert sorted(p[:3]) == [1, 2, 3]
    got = RO.beam_search(sc, (0,), 3, 1, exclude=(0, 1, 2))            # one candidate: two dead beams from step 0
    assert got["paths"][:, 0].tolist() == [3, -1, -1] and np.isfinite(got["total"][0]) and np.isneginf(got["total"][1:]).all()


def test_header_declares_both_entries_and_the_source_is_built():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("poi_route_expand", "poi_route_merge"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in poi_amd._lib.SIGNATURES
    assert "route.hip" in poi_amd.build.SOURCES
    for key in ("route_path", "route_splits"):
        assert key in poi_amd._lib.PLAN_KEYS and '"%s"' % key in hdr
    assert '"route_split_max"' in hdr and '"route_grid"' in hdr and '"route_expand"' in hdr and '"route_merge"' in hdr


def test_host_argument_checks():
    assert M.Session._route_args(16, 8) == (16, 8) and M.Session._route_args(1, 1) == (1, 1)
    for steps, beam in ((4, 9), (4, 0), (17, 4), (0, 4), (-1, 4)):
        with pytest.raises(M._lib.PoiError):
            M.Session._route_args(steps, beam)
    carnn = M.CellSession.__new__(M.CellSession)                        # (no device: the refusal comes before anything is touched)
    carnn.carnn = True
    with pytest.raises(M._lib.PoiError, match="OboCARNN"):
        carnn.recommend_route([0], 3)


@pytest.mark.parametrize("kind,name", RC.FIXTURES)
def test_fixtures_have_clear_decisions(kind, name):
    R = RC.solve(kind, name)
    share = float(R["clear"].mean())
    print("%s %s %s: %.0f %% of %d slots are clear, max|score| %.2f" % (kind, name, RC.SHAPES[name], 100 * share, len(R["clear"]), R["max_abs"]))
    assert share >= RC.CLEAR_MIN, "%s %s: only %.1f %% of the slots are clear: pick another seed or shape" % (kind, name, 100 * share)
