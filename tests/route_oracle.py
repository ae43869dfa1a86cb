"""float64 numpy oracle of the route recommendation (include/poi_hip.h, route recommendation): a beam search over a slot's next POIs by
the definition, written for clarity.  Every hypothesis is scored by running the oracle's `predict` on history + path from the
float32-rounded tables (oracle.poi_oracle.spatial_predict / gru_predict and the `oracle_scores` rule of tests/test_gpu_session.py;
tests/session_cells_oracle.py for Lstm / Rnn).  The search also records every gap a float32 kernel has to resolve, so that the tests
can tell - on the oracle alone - which slots a correct kernel must reproduce exactly."""
import numpy as np

from oracle import poi_oracle as O
from tests import session_cells_oracle as S
from tests.test_gpu_session import oracle_rows, oracle_scores

RES = 1e-6          # the project's ranking resolution: 1e-6 max|score| (tests/test_gpu_fullsize.py)


class Scorer:
    """scores(seq) -> float64 scores of every POI for the state after the check-ins `seq` (memoised).  kind: "spatial", "plain", "lstm",
    "rnn".  An empty sequence is a fresh slot: h = 0 and no distance term, every score 0."""

    def __init__(self, kind, P, T):
        self.kind, self.P, self.T = kind, P, T
        self.n_item = T["n_item"]
        self.memo = {}
        self.max_abs = 0.0

    def scores(self, seq):
        seq = tuple(int(v) for v in seq)
        if seq not in self.memo:
            P, T = self.P, self.T
            if not seq:
                sc = np.zeros(self.n_item)
            elif self.kind in ("lstm", "rnn"):
                h, _ = S.cell_prefix_states(P, self.kind, seq)
                sc = O.score_all(h[-1:], P["lt"])[0]
            else:
                hts, sts = oracle_rows(P, T, [seq], spatial=self.kind == "spatial")
                sc = oracle_scores(P, T, hts, sts, [seq[-1]])[0]
            self.memo[seq] = sc
            self.max_abs = max(self.max_abs, float(np.abs(sc[~np.isnan(sc)]).max()))
        return self.memo[seq]


def lse(sc):
    """log sum exp over all POIs, NaN scores left out."""
    v = sc[~np.isnan(sc)]
    m = v.max()
    return m + np.log(np.sum(np.exp(v - m)))


def candidates(sc, n_item, exclude, path, revisit):
    """Candidate ids by descending score, ties by ascending id."""
    ok = ~np.isnan(sc)
    ok[np.asarray(list(exclude), np.int64)] = False
    if not revisit:
        ok[np.asarray(list(path), np.int64)] = False
    ids = np.nonzero(ok)[0]
    return ids[np.lexsort((ids, -sc[ids]))]


def beam_search(scorer, history, beam, steps, exclude=(), revisit=False):
    """-> dict(paths (beam, steps) int64 with -1 where dead, total (beam) with -inf where dead, steplp (beam, steps) with -inf where dead,
    gaps: list of (t, gap) - at step t the adjacent gaps among each live hypothesis's best beam + 1 candidate scores and among the
    slot's best beam + 1 merged totals)."""
    history = tuple(int(v) for v in history)
    n_item = scorer.n_item
    hyps = [((), 0.0, ())]                           # live hypotheses: (path, total, step log-probabilities)
    paths = np.full((beam, steps), -1, np.int64)
    steplp = np.full((beam, steps), -np.inf)
    total = np.full(beam, -np.inf)
    gaps = []
    for t in range(steps):
        props = []
        for bi, (path, tot, slp) in enumerate(hyps):
            sc = scorer.scores(history + path)
            z = lse(sc)
            order = candidates(sc, n_item, exclude, path, revisit)
            top = sc[order[:beam + 1]]
            gaps += [(t, float(g)) for g in top[:-1] - top[1:]]
            props += [(tot + (sc[j] - z), bi, int(j), sc[j] - z) for j in order[:beam]]
        props.sort(key=lambda x: (-x[0], x[1], x[2]))
        tt = np.array([x[0] for x in props[:beam + 1]])
        gaps += [(t, float(g)) for g in tt[:-1] - tt[1:]]
        old = hyps
        hyps = [(old[bi][0] + (j,), tot, old[bi][2] + (lp,)) for tot, bi, j, lp in props[:beam]]
        # a place without a proposal is dead from here on and keeps the prefix of its own place
        prev_paths, prev_lp = paths.copy(), steplp.copy()
        for k in range(beam):
            if k < len(hyps):
                paths[k, :t + 1] = hyps[k][0]; steplp[k, :t + 1] = hyps[k][2]; total[k] = hyps[k][1]
            else:
                src = min(k, len(old) - 1) if t == 0 else k
                paths[k, :t] = prev_paths[src, :t]; steplp[k, :t] = prev_lp[src, :t]
                paths[k, t] = -1; steplp[k, t] = -np.inf; total[k] = -np.inf
        if not hyps:
            break
    return dict(paths=paths, total=total, steplp=steplp, gaps=gaps)


def path_logp(scorer, history, path):
    """Total log-probability of a given path (ids >= 0): sum_t s(state_t, path[t]) - lse(state_t); also the per-step terms."""
    history = tuple(int(v) for v in history)
    out = []
    for t, j in enumerate(path):
        sc = scorer.scores(history + tuple(int(v) for v in path[:t]))
        out.append(sc[int(j)] - lse(sc))
    return float(np.sum(out)), np.array(out)


def clear(gaps, max_abs):
    """Every decision of a slot was clear: each gap of step t is at least 4 (t + 1) RES max|score| - the ranking resolution charged once
    for the score and once for the normaliser per step, for both sides of a comparison."""
    return all(g >= 4 * (t + 1) * RES * max_abs for t, g in gaps)


def brute_force(scorer, history, beam, steps, exclude=(), revisit=False):
    """The same search by enumerating every path: the log-probability of every prefix of length t + 1 that extends a kept prefix is
    computed from scratch, each kept parent keeps its best `beam` children, the slot its best `beam` overall."""
    import itertools
    history = tuple(int(v) for v in history)
    n_item = scorer.n_item
    kept = [()]
    for t in range(steps):
        full = {}
        for path in itertools.product(range(n_item), repeat=t + 1):
            if path[:t] not in kept or path[t] in exclude or (not revisit and path[t] in path[:t]):
                continue
            full[path] = path_logp(scorer, history, path)[0]
        props = []
        for bi, par in enumerate(kept):
            sc = scorer.scores(history + par)
            kids = sorted((p for p in full if p[:t] == par), key=lambda p: (-sc[p[t]], p[t]))[:beam]
            props += [(full[p], bi, p[t], p) for p in kids]
        props.sort(key=lambda x: (-x[0], x[1], x[2]))
        kept = [x[3] for x in props[:beam]]
        totals = [x[0] for x in props[:beam]]
        if not kept:
            break
    return kept, totals
