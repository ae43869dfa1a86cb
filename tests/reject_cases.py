"""Rejection placements shared by the sort-based training steps (csrc/bpr.hip, fpmc.hip, prme.hip, vbpr.hip; geoie.hip and poi2vec.hip
reject whole users: user_cases below).  Contract of include/poi_hip.h: an element with an id outside its table (or p == q, a bad distance,
...) moves nothing, gets a NaN loss and is counted once - the launch equals the launch WITHOUT it, bit for bit.  The kernels give a rejected
element's touches a sentinel key that sorts last; the placements here are the ones where a sorted scatter over 64-touch windows goes wrong:

  first / last      a rejected element at position 0 / at position n - 1
  edge-1 / edge / edge+1   WINDOW[step] kept elements (one fewer, one more) whose valid touches fill whole 64-touch windows of every sorted
                    part exactly, so that the sentinel run starts on a window start (before it, after it)
  long_run          LONG consecutive rejected elements: a sentinel run longer than a window in every part
  all_rejected, n1  nothing kept: LONG elements, and the launch of one
  sole              rejected elements (one per kind) whose VALID ids name only the reserved rows: rows no kept element touches
  all_bad           one element with every id out of range (negative, n, n + 1, 1 << 20)
  kind:<k>          one rejected element of each kind the step's header lists, a copy of a kept element (its valid ids name SHARED rows)

Every case reserves the last two user rows and the last three POI rows + the pad row: no kept element names them (user n_user - 1 and the
pad row n_item are where the clamped keys of the old csrc/bpr.hip landed).  numpy only; tests/test_reject_cases_cpu.py checks the fixture
conditions, tests/test_gpu_rejected.py runs the cases."""
from collections import namedtuple

import numpy as np

N_USER, N_ITEM = 40, 100          # tables of 40 and 101 rows
N_CLEAN, LONG = 200, 70
RES_USER = np.array([N_USER - 2, N_USER - 1])
RES_POI = np.array([N_ITEM - 3, N_ITEM - 2, N_ITEM - 1, N_ITEM])

Spec = namedtuple("Spec", "user poi extras parts window kinds")
# parts: the sorted parts of the step's touch array, each a tuple of (table, id field) touches per element (BPR sorts its user and POI
# touches apart, the others one array over all tables)
SPECS = {
    "bpr": Spec("u", ("p", "q"), (), (((0, "u"),), ((1, "p"), (1, "q"))), 64, ("u", "p", "q")),
    "fpmc": Spec("u", ("a", "i", "j"), (), (((0, "u"), (1, "a"), (2, "i"), (2, "j"), (3, "i"), (3, "j")),), 32, ("u", "a", "i", "j", "i==j")),
    "prme": Spec("u", ("p", "q", "prev"), ("d", "gap"), (((0, "u"), (1, "p"), (1, "q"), (1, "prev"), (2, "p"), (2, "q"), (2, "prev")),), 64,
                 ("u", "p", "q", "prev", "p==q", "d_nan", "d_neg", "d_inf")),
    "vbpr": Spec("u", ("p", "q"), (), (((0, "u"), (1, "u"), (2, "p"), (2, "q")),), 16, ("u", "p", "q", "p==q")),
}
WINDOW = {k: s.window for k, s in SPECS.items()}

Case = namedtuple("Case", "name launch keep rejected res_user res_poi")


def bad_user(v):
    return (N_USER, -1, N_USER + 1, 1 << 20)[v % 4]


def bad_poi(v):
    """the pad row N_ITEM is a legal id: the table has N_ITEM + 1 rows"""
    return (N_ITEM + 1, -2, N_ITEM + 2, 1 << 20)[v % 4]


def is_rejected(step, e):
    s = SPECS[step]
    if not 0 <= e[s.user] < N_USER or any(not 0 <= e[f] <= N_ITEM for f in s.poi):
        return True
    if step == "fpmc" and e["i"] == e["j"]:
        return True
    if step in ("prme", "vbpr") and e["p"] == e["q"]:
        return True
    return step == "prme" and not (np.isfinite(e["d"]) and e["d"] >= 0)


def _clean(step, rng, n, full=False, disjoint=False):
    """n kept elements: users < N_USER - 2, POIs < N_ITEM - 3, half of the draws on a few hot rows (shared rows, long runs); the POI ids
    of one element are distinct.  full: every element has all its touches (PRME: prev is neither p nor q, no lost occurrence).
    disjoint: no row is named twice in the whole launch (BPR's racy mode equals the reference there)."""
    s = SPECS[step]
    nu, ni, k = N_USER - 2, N_ITEM - 3, len(s.poi)
    out = []
    if disjoint:
        assert n <= nu and k * n <= ni
        us, ps = rng.permutation(nu), rng.permutation(ni)
    for t in range(n):
        if disjoint:
            e = {s.user: int(us[t])}
            e.update({f: int(ps[k * t + c]) for c, f in enumerate(s.poi)})
        else:
            e = {s.user: int(rng.integers(0, 4) if rng.random() < 0.5 else rng.integers(0, nu))}
            ids = []
            while len(ids) < k:
                v = int(rng.integers(0, 5) if rng.random() < 0.5 else rng.integers(0, ni))
                if v not in ids:
                    ids.append(v)
            e.update(dict(zip(s.poi, ids)))
            if step == "prme" and not full and t % 16 == 5:
                e["prev"] = e["p"]                       # a repeated check-in: the p occurrence is lost (keyed as the sentinel too)
            if step == "fpmc" and t % 16 == 9:
                e["a"] = e["i"]                          # rows of different tables
        if step == "prme":
            e["d"] = float(rng.exponential(3.0))
            e["gap"] = 1000 if rng.random() < 0.3 else 20
        out.append(e)
    return out


def reject(step, base, kind, v=0, sole=False):
    """a rejected copy of the kept element `base`; sole: its valid ids are moved onto the reserved rows"""
    s = SPECS[step]
    e = dict(base)
    if sole:
        e[s.user] = int(RES_USER[0])
        for c, f in enumerate(s.poi):
            e[f] = int(RES_POI[c])
    if kind == "all":
        e[s.user] = bad_user(v)
        for c, f in enumerate(s.poi):
            e[f] = bad_poi(v + 1 + c)
    elif kind == s.user:
        e[kind] = bad_user(v)
    elif kind in s.poi:
        e[kind] = bad_poi(v)
    elif "==" in kind:
        a, b = kind.split("==")
        e[b] = e[a]
    else:
        e["d"] = {"d_nan": np.nan, "d_neg": -0.5, "d_inf": np.inf}[kind]
    assert is_rejected(step, e), (step, kind, e)
    return e


def _case(step, name, elems):
    s = SPECS[step]
    fields = (s.user,) + s.poi + s.extras
    launch = {f: np.array([e[f] for e in elems], np.float64 if f == "d" else np.int64) for f in fields}
    rej = np.array([is_rejected(step, e) for e in elems], bool)
    return Case(name, launch, np.nonzero(~rej)[0], np.nonzero(rej)[0], RES_USER, RES_POI)


def build(step, seed=0, disjoint=False):
    """{name: Case} for one of SPECS.  disjoint: the kept elements share no row (no window-edge cases: the tables are too small for them)."""
    s = SPECS[step]
    rng = np.random.default_rng(1000 + seed)
    n = 30 if disjoint else N_CLEAN
    clean = _clean(step, rng, n, disjoint=disjoint)
    kinds = s.kinds
    rj = lambda t, i, **kw: reject(step, clean[t % n], kinds[i % len(kinds)], v=i, **kw)
    cases = [_case(step, "first", [rj(3, 0)] + clean), _case(step, "last", clean + [rj(5, 1)])]
    if not disjoint:
        for d in (-1, 0, 1):
            kept = _clean(step, rng, s.window + d, full=True)
            mid = len(kept) // 2
            elems = [reject(step, kept[1], kinds[0], 1)] + kept[:mid] + [reject(step, kept[2], kinds[1], 2)] + kept[mid:] + \
                [reject(step, kept[3], kinds[-1], 3)]
            cases.append(_case(step, "edge%s" % ("%+d" % d if d else ""), elems))
    h = n // 2
    cases.append(_case(step, "long_run", clean[:h] + [rj(t, t) for t in range(LONG)] + clean[h:]))
    cases.append(_case(step, "all_rejected", [rj(t, t) for t in range(LONG)]))
    cases.append(_case(step, "n1", [rj(0, 0)]))
    sole = [reject(step, clean[7 % n], k, v=i, sole=True) for i, k in enumerate(kinds)]
    cases.append(_case(step, "sole", clean[:h] + sole[:1] + clean[h:] + sole[1:]))
    cases.append(_case(step, "all_bad", clean[:h] + [reject(step, clean[0], "all", 1)] + clean[h:]))
    t = 77 % n
    for i, k in enumerate(kinds):
        cases.append(_case(step, "kind:" + k, clean[:t] + [reject(step, clean[t], k, v=i)] + clean[t:]))
    return {c.name: c for c in cases}


def take(launch, idx):
    return {f: v[idx] for f, v in launch.items()}


def part_keys(step, launch):
    """The keys of the step's touches, one int64 array per sorted part, as the kernels build them: (table, row) in one key space per part,
    -1 for a touch keyed as the sentinel (every touch of a rejected element; PRME's lost occurrences)."""
    s = SPECS[step]
    n = len(launch[s.user])
    rej = np.array([is_rejected(step, {f: v[t] for f, v in launch.items()}) for t in range(n)], bool)
    R = N_ITEM + 1
    out = []
    for part in s.parts:
        keys = []
        for table, f in part:
            lost = rej.copy()
            if step == "prme" and f in ("p", "q"):
                lost |= launch[f] == launch["prev"]
            keys.append(np.where(lost, -1, table * (N_USER + R) + launch[f].astype(np.int64)))
        out.append(np.concatenate(keys))
    return out


def named_rows(step, launch, idx):
    """(user rows, POI rows) named by the elements idx"""
    s = SPECS[step]
    pois = np.concatenate([launch[f][idx] for f in s.poi]) if len(idx) else np.zeros(0, np.int64)
    return np.unique(launch[s.user][idx]), np.unique(pois)


# ---- steps that reject whole users (geoie.hip, poi2vec.hip) ------------------------------------------------------------------------
UserCase = namedtuple("UserCase", "name users keep rejected")


def user_cases(good, bad):
    """Placements of rejected users in a launch of user ids.  good: ids of users the step accepts (at most 40); bad: {kind: user id} of
    users it rejects (an id outside the table, a user with an out-of-range target, ...).  -> {name: UserCase}."""
    good = list(good)
    kinds = sorted(bad)
    cyc = lambda i: bad[kinds[i % len(kinds)]]
    h = len(good) // 2
    raw = [("first", [cyc(0)] + good), ("last", good + [cyc(1)]),
           ("long_run", good[:h] + [cyc(i) for i in range(LONG)] + good[h:]),
           ("all_rejected", [cyc(i) for i in range(LONG)]), ("n1", [cyc(0)])]
    raw += [("kind:" + k, good[:h] + [bad[k]] + good[h:]) for k in kinds]
    badset = set(bad.values())
    out = {}
    for name, users in raw:
        users = np.asarray(users, np.int64)
        rej = np.array([int(u) in badset for u in users], bool)
        out[name] = UserCase(name, users, np.nonzero(~rej)[0], np.nonzero(rej)[0])
    return out
