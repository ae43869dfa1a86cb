"""CPU checks of the re-ranking tests' own tools: the numpy oracle (tests/rerank_oracle.py) on an example worked by hand and against a
brute-force sort, the fixtures of tests/rerank_cases.py (they contain what they claim), the declarations of the new entries, the host
side argument checks of the Python layer, and evaluate.two_stage_metrics on two oracle-scored stand-in models.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import rerank_cases as RC
from tests import rerank_oracle as RO
from tests import select_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_oracle_on_an_example_worked_by_hand():
    """ids 7 3 7 -1 5, scores 1 2 1 9 NaN: the padding and the NaN leave; 3 (score 2) leads; the two 7s tie and the position decides."""
    ids = np.array([7, 3, 7, -1, 5], np.int32)
    sc = np.array([1.0, 2.0, 1.0, 9.0, np.nan], np.float32)
    oi, ov, op, cnt, bad = RO.rerank(np.array([0, 5]), ids, 1, sc, 4)
    assert oi.tolist() == [[3, 7, 7, -1]] and op.tolist() == [[1, 0, 2, -1]] and cnt.tolist() == [3] and bad == 0
    assert ov[0, :3].tolist() == [2.0, 1.0, 1.0] and np.isneginf(ov[0, 3])
    # a blend: 0.5 * score + 0.25 * prior with priors 0 -4 4 0 0 -> keys 0.5, 0, 1.5: the second 7 leads, then the first, then 3
    pr = np.array([0.0, -4.0, 4.0, 0.0, 0.0], np.float32)
    oi, ov, op, cnt, _ = RO.rerank(np.array([0, 5]), ids, 1, sc, 2, pr, (0.5, 0.25))
    assert oi.tolist() == [[7, 7]] and op.tolist() == [[2, 0]] and ov.tolist() == [[1.5, 0.5]] and cnt.tolist() == [3]
    # both zeros are one key (the id decides) and come out as +0.0; +inf is selectable, -inf is not
    ids = np.array([4, 2, 9, 1], np.int32)
    sc = np.array([0.0, -0.0, np.inf, -np.inf], np.float32)
    oi, ov, op, cnt, _ = RO.rerank(None, ids, 1, sc[None, :], 4)
    assert oi.tolist() == [[9, 2, 4, -1]] and cnt.tolist() == [3] and not np.signbit(ov[0, 1]) and not np.signbit(ov[0, 2])
    # the key arithmetic is float64 then float32: 1 + 2^-30 is kept by the sum and lost by the rounding to float32
    t = RO.key_of(np.array([1.0], np.float32), np.array([2.0 ** -30], np.float32), (1.0, 1.0))
    assert t.dtype == np.float32 and t[0] == np.float32(1.0)


def test_score_lists_oracle_rules():
    full = np.arange(12, dtype=np.float32).reshape(2, 6)
    off, cand = RO.csr([[5, -1, 0, 5], [1]])
    s, bad = RO.score_lists(full, off, cand)
    assert bad == 0 and s[[0, 2, 3, 4]].tolist() == [5.0, 0.0, 5.0, 7.0] and np.isneginf(s[1])
    s, bad = RO.score_lists(full, off, np.array([5, -1, 6, 5, 1]))      # row 0 holds an id beyond the table
    assert bad == 1 and np.isneginf(s[:4]).all() and s[4] == 7.0
    for broken in ([0, 5, 4], [-1, 4, 5], [0, 4, 6]):                   # descending, negative, beyond n_cand
        s, bad = RO.score_lists(full, np.array(broken), cand)
        assert bad >= 1
    s, bad = RO.score_lists(full, None, np.array([0, 6]))
    assert bad == 1 and np.isneginf(s).all() and s.shape == (2, 2)
    s, bad = RO.score_lists(full, None, np.array([3, -1, 3]))
    assert bad == 0 and s[:, 0].tolist() == [3.0, 9.0] and np.isneginf(s[:, 1]).all() and np.array_equal(s[:, 0], s[:, 2])
    off, flat = RO.csr_of_padded(np.array([[1, -1], [2, 3]]))
    assert off.tolist() == [0, 2, 4] and flat.tolist() == [1, -1, 2, 3]


@pytest.mark.parametrize("shape", ["short", "odd", "s_small"])
def test_the_oracle_is_a_brute_force_sort(shape):
    F = RC.any_fixture(shape)
    for with_prior in (False, True):
        ids, val, pos, cnt, _ = RC.expected(shape, with_prior)
        t = RO.key_of(F["score"], F["prior"] if with_prior else None, RC.WEIGHTS)
        for r in range(F["n"]):
            if F["off"] is None:
                row_ids, row_t = F["cand"], t[r]
            else:
                row_ids, row_t = F["cand"][F["off"][r]:F["off"][r + 1]], t[F["off"][r]:F["off"][r + 1]]
            want = RO.brute_force_row(row_ids, row_t, 64)
            assert [(int(a), int(b)) for a, b in zip(ids[r, :len(want)], pos[r, :len(want)])] == want, (shape, with_prior, r)
            assert cnt[r] >= len(want) and (len(want) == 64 or ids[r, len(want)] == -1)


def test_the_fixtures_contain_what_they_claim():
    assert RC.CHUNK - 1 in RC.LENGTHS and RC.CHUNK in RC.LENGTHS and RC.CHUNK + 1 in RC.LENGTHS
    assert {0, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4096} <= set(RC.LENGTHS) and RC.TOO_LONG == 4097
    assert {v[0] for v in RC.SHAPES.values()} == {1, 31, 32, 33, 70, 300} and {v[1] for v in RC.SHAPES.values()} == {13, 1037, 5000}
    seen_len, tie_at_k, dup_pair, dead, short, mid_pad, blend_tie = set(), 0, 0, 0, 0, 0, 0
    for shape in RC.SHAPES:
        F = RC.fixture(shape)
        L = RC.lengths(F)
        seen_len |= set(L.tolist())
        assert F["cand"].max() < F["n_item"] and len(F["score"]) == len(F["prior"]) == len(F["cand"]) == F["off"][-1]
        for with_prior in (False, True):
            ids, val, pos, cnt, bad = RC.expected(shape, with_prior)
            assert bad == F["bad"]
            for r in range(F["n"]):
                c = int(cnt[r])
                if L[r] > RO.LEN_MAX:
                    assert c == 0 and (ids[r] == -1).all()
                    continue
                dead += L[r] > 0 and c == 0
                short += 0 < c < 20 and L[r] >= 20
                if c > 20 and val[r, 19] == val[r, 20]:
                    tie_at_k += 1                    # a tie straddling place k = 20
                    blend_tie += with_prior and ids[r, 19] != ids[r, 20]
                same = (ids[r, :c - 1] == ids[r, 1:c]) & (val[r, :c - 1] == val[r, 1:c]) if c > 1 else np.zeros(0, bool)
                if same.any():
                    dup_pair += 1
                    i = int(np.nonzero(same)[0][0])
                    assert pos[r, i] < pos[r, i + 1]                 # duplicates of one id with one key: the position decides
            row_ids = [F["cand"][F["off"][r]:F["off"][r + 1]] for r in range(F["n"])]
            mid_pad += sum(1 for x in row_ids if len(x) >= 3 and (x[1:-1] < 0).any())
    assert seen_len == set(RC.LENGTHS) | {RC.TOO_LONG}
    assert min(tie_at_k, dup_pair, dead, short, mid_pad, blend_tie) >= 3, (tie_at_k, dup_pair, dead, short, mid_pad, blend_tie)
    for shape, (n, N, C) in RC.SHARED.items():
        F = RC.shared_fixture(shape)
        assert F["score"].shape == F["prior"].shape == (n, C) and F["cand"].shape == (C,) and F["cand"].max() < N
    assert RC.SHARED["s_max"][2] == RO.LEN_MAX
    off, cand = RC.scoring_lists(80, 1037, 20)
    assert set(np.diff(off).tolist()) == {L for L in RC.LENGTHS if L <= 1025} and (cand < 0).any() and cand.max() < 1037


def test_entry_points_are_declared_bound_and_built():
    import poi_amd
    from poi_amd import evaluate as E
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    for name, n_args in (("poi_score_lists_chunk", 0), ("poi_score_lists", 19), ("poi_rerank_lists", 15), ("poi_rerank", 26)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/poi_hip.h" % name
        assert name in poi_amd._lib.SIGNATURES, "%s has no ctypes binding" % name
        declared = 0 if m.group(1).strip() == "void" else m.group(1).count(",") + 1
        assert len(poi_amd._lib.SIGNATURES[name][1]) == declared == n_args, "%s: argument counts differ" % name
    assert re.search(r"additive to 9: re-ranking - new entry points poi_score_lists, poi_rerank_lists and poi_rerank", hdr)
    assert re.search(r"#define POI_ABI_VERSION 9\b", hdr) and poi_amd._lib.ABI_VERSION == 9
    assert hdr.index("additive to 9: re-ranking") < hdr.index("#define POI_ABI_VERSION 9")
    assert "rerank.hip" in poi_amd.build.SOURCES
    assert "lists_path" in poi_amd._lib.PLAN_KEYS and '"lists_path"' in hdr
    for name in ('"score_lists"', '"rerank_lists"', '"rerank"'):
        assert name in hdr
    for cls in (poi_amd.models._Base, poi_amd.models.Session, poi_amd.models.CellSession):
        assert callable(getattr(cls, "rerank")) and callable(getattr(cls, "score_lists"))
    assert callable(E.two_stage_metrics)


def bare_model(n_item=50):
    """A _Base without tables or a device context: what the host-side argument checks read."""
    import torch
    import poi_amd
    m = object.__new__(poi_amd.models._Base)
    m.device, m.n_item = torch.device("cpu"), n_item
    return m


def test_host_side_argument_errors():
    import torch
    m = bare_model(50)
    n = 3
    L = m._rerank_lists_arg(np.array([[1, 2, -1], [3, 3, 4], [-1, -1, -1]]), n)
    assert L["off"].tolist() == [0, 3, 6, 9] and L["n_cand"] == 9 and L["shape"] == (3, 3) and L["ids"].dtype == torch.int32
    L = m._rerank_lists_arg((np.array([0, 2, 2, 5]), np.array([1, 2, 3, 4, 49])), n)
    assert L["shape"] is None and L["n_cand"] == 5
    L = m._rerank_lists_arg(np.arange(7), n)
    assert L["off"] is None and L["shape"] == (3, 7)
    L0 = m._rerank_lists_arg((np.zeros(4, np.int64), np.zeros(0, np.int64)), n)
    assert L0["n_cand"] == 0 and L0["ids"].numel() == 1                 # an empty id array still has an address
    with pytest.raises(IndexError):
        m._rerank_lists_arg(np.array([[1, 50, 2]] * 3), n)               # an id beyond the table
    with pytest.raises(IndexError):
        m._rerank_lists_arg(np.array([50]), n)
    for off in ([0, 2, 1, 5], [-1, 2, 3, 5], [0, 2, 3, 6]):              # descending, negative, beyond the ids
        with pytest.raises(ValueError):
            m._rerank_lists_arg((np.array(off), np.arange(5)), n)
    with pytest.raises(ValueError):
        m._rerank_lists_arg((np.array([0, 5]), np.arange(5)), n)        # n + 1 offsets
    with pytest.raises(ValueError):
        m._rerank_lists_arg(np.zeros((2, 4), np.int64), n)               # (n, C)
    with pytest.raises(ValueError):
        m._rerank_lists_arg(np.zeros((3, 2, 2), np.int64), n)
    L = m._rerank_lists_arg(np.array([[1, 2, -1], [3, 3, 4], [-1, -1, -1]]), n)
    for k in (0, -1, 4097):
        with pytest.raises(ValueError):
            m._rerank_args(L, n, k, None, (1.0, 0.0))
    with pytest.raises(ValueError):
        m._rerank_args(L, n, 5, np.zeros(8, np.float32), (1.0, 0.0))     # one prior per entry
    with pytest.raises(ValueError):
        m._rerank_args(L, n, 5, None, (1.0,))
    with pytest.raises(ValueError):
        m._rerank_args(m._rerank_lists_arg(np.arange(4097) % 50, n), n, 5, None, (1.0, 0.0))       # a shared list beyond 4096
    with pytest.raises(ValueError):
        m._rerank_args(m._rerank_lists_arg((np.array([0, 4097, 4097, 4097]), np.zeros(4097, np.int64)), n), n, 5, None, (1.0, 0.0))
    k, prior, w = m._rerank_args(L, n, 9, np.arange(9.0), (2, 3))
    assert k == 9 and prior.dtype == torch.float32 and prior.shape == (9,) and w == (2.0, 3.0)


class StandIn:
    """What evaluate.two_stage_metrics reads of a model, scored by the oracles from a given float32 matrix on torch's CPU device."""

    def __init__(self, sc, tgt, tm, train):
        import torch
        self.sc, self.train = np.asarray(sc, np.float32), train
        self.n_user, self.n_item = self.sc.shape
        self.device = torch.device("cpu")
        self.tes_buys_masks, self.tes_masks = torch.as_tensor(tgt.astype(np.int32)), torch.as_tensor(tm.astype(np.int32))

    def _ids(self, se):
        import torch
        return torch.as_tensor(np.asarray(se).astype(np.int32)), None

    def _rows(self, table, ids, lo):
        return table.index_select(0, ids.long())

    def _ex(self, rows, exclude):
        return SO.csr([self.train[r] for r in rows]) if exclude == "train" else (None, None)

    def compute_sub_target_rank(self, se, exclude=None, targets=None):
        import torch
        rows = np.asarray(se)
        tgt, tm = (t.numpy() for t in targets)
        out = np.full(tgt.shape, -1, np.int64)
        for i, r in enumerate(rows):
            gone = set(self.train[r].tolist()) if exclude == "train" else set()
            s = self.sc[r].astype(np.float64)
            for j in range(tgt.shape[1]):
                t = int(tgt[i, j])
                if tm[i, j] and t not in gone:
                    out[i, j] = sum(1 for q in range(self.n_item) if q != t and q not in gone and (s[q] > s[t] or (s[q] == s[t] and q < t)))
        return torch.as_tensor(out.astype(np.int32))

    def compute_sub_candidates(self, se, k, exclude=None):
        import torch
        rows = np.asarray(se)
        return torch.as_tensor(SO.select(self.sc[rows], k, *self._ex(rows, exclude))[0])

    def rerank(self, se, lists, k):
        import torch
        rows = np.asarray(se)
        off, cand = RO.csr_of_padded(lists.numpy())
        s, bad = RO.score_lists(self.sc[rows], off, cand)
        assert bad == 0
        return torch.as_tensor(RO.rerank(off, cand, len(rows), s, k)[0])


def test_two_stage_metrics_on_stand_in_models():
    from poi_amd import evaluate as E
    rng = np.random.default_rng(5)
    n, N = 24, 60
    good = rng.normal(size=(n, N)).astype(np.float32)
    noisy = (good + 0.8 * rng.normal(size=(n, N))).astype(np.float32)
    train = [np.sort(rng.choice(N, 5, replace=False)) for _ in range(n)]
    tgt = np.stack([np.argsort(-np.where(np.isin(np.arange(N), train[r]), -np.inf, good[r]))[[0, 7]] for r in range(n)])
    tm = np.ones_like(tgt); tm[3, 1] = 0
    ranker, retriever = StandIn(good, tgt, tm, train), StandIn(noisy, tgt, tm, train)
    se = [np.arange(0, 10), np.arange(10, n)]
    same = E.two_stage_metrics(ranker, ranker, se, cands=(10, 30), ks=(1, 5, 10))
    for c in (10, 30):
        assert same[c]["agreement"] == {1: 1.0, 5: 1.0, 10: 1.0} and same[c]["two_stage"]["recall"] == same[c]["ranker"]["recall"]
        assert same[c]["ranker"]["recall"] == {1: 24 / 47, 5: 24 / 47, 10: 1.0}      # the targets are the ranker's ranks 0 and 7
    assert abs(same[30]["ranker"]["mrr"] - (24 + 23 / 8) / 47) < 1e-12
    got = E.two_stage_metrics(retriever, ranker, se, cands=(10, 30, 55), ks=(1, 5, 10))
    assert got[55]["agreement"] == {1: 1.0, 5: 1.0, 10: 1.0}            # every POI that is not excluded is a candidate: the ranker's order
    assert got[55]["two_stage"] == {"mrr": got[55]["ranker"]["mrr"], "recall": got[55]["ranker"]["recall"]}
    assert got[10]["agreement"][10] < 1.0 and got[10]["two_stage"]["recall"][10] <= got[30]["two_stage"]["recall"][10] <= 1.0
    assert got[10]["retriever"]["mrr"] < got[10]["ranker"]["mrr"] and got[10]["two_stage"]["mrr"] <= got[10]["ranker"]["mrr"]
    # a held-out POI inside the candidates has the ranker's place among them: the two-stage recall at c is the retriever's recall at c
    r10 = E.two_stage_metrics(retriever, ranker, se, cands=(10,), ks=(10,))[10]
    assert r10["two_stage"]["recall"][10] == r10["retriever"]["recall"][10]
    for bad in (dict(cands=(30, 10)), dict(ks=(5, 5)), dict(cands=(10, 30), ks=(20,)), dict(cands=(0,))):
        with pytest.raises(ValueError):
            E.two_stage_metrics(retriever, ranker, se, **bad)
    with pytest.raises(ValueError):
        E.two_stage_metrics(StandIn(good[:, :50], tgt, tm, train), ranker, se)
