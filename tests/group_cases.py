"""The problems of tests/test_gpu_group.py, built on the host: tests/test_group_cpu.py checks on the CPU that the oracle alone ranks
them with clear gaps, the GPU tests build the models from them.  Cases come from make_case of tests/test_gpu_near.py."""
import functools

import numpy as np

from tests import group_oracle as GO
from tests.test_gpu_near import last_of, make_case

K = 20
N_USER, N_ITEM = 80, 1037
SIZES = (1, 2, 15, 16, 17, 32, 33, 70)              # below / at / above half a tile and a tile of 32 member rows; several chunks
NO_LAST = (3, 11, 40, 77)                            # spatial: members without a last POI (no distance term)
# kind, dim: FPMC-LR scores at kdim = 2 dim, so its dim 256 (kdim 512) is beyond the kernels' dim <= 256
RANK_CASES = [(kind, dim) for kind in ("bpr", "spatial", "fpmc") for dim in (4, 20, 128, 256) if (kind, dim) != ("fpmc", 256)]


def mixed_groups(seed, n_user=N_USER):
    """The sizes of SIZES in one call, a repeated member, an empty group and a few small parties: 19 groups, three workgroups' worth."""
    rng = np.random.default_rng(seed)
    groups = [rng.choice(n_user, s, replace=False) for s in SIZES]
    groups.append(np.array([5, 9, 5, 3]))            # a member listed twice counts twice
    groups.append(np.zeros(0, np.int64))             # an empty group
    groups += [rng.choice(n_user, s, replace=False) for s in (4, 4, 3, 5, 4, 2, 6, 4, 33)]
    return groups


def exclusion_lists(seed, n_grp, n_item):
    """One ascending list per group: some empty, some long."""
    rng = np.random.default_rng(seed + 1)
    lists = [np.sort(rng.choice(n_item, rng.integers(0, 60), replace=False)) if g % 3 else np.zeros(0, np.int64) for g in range(n_grp)]
    return GO.csr(lists)


@functools.lru_cache(maxsize=None)
def rank_case(kind, dim):
    """dict(C (make_case), last (the members' last POIs, -1 for NO_LAST on the spatial case), sc (member scores), off, ids, ex)."""
    C = make_case(kind, dim, 300 + dim, n_user=N_USER, n_item=N_ITEM)
    T = C["T"]
    last = last_of(T).astype(np.int64)
    if kind == "spatial":
        last[list(NO_LAST)] = -1
        sc = GO.member_scores(C["users"], C["items"], last, C["term"][0], C["term"][1], T["coords"], T["dd_m"], T["n_dist"])
    else:
        sc = GO.member_scores(C["users"], C["items"])
    off, ids = GO.csr(mixed_groups(dim))
    return dict(C=C, last=last, sc=sc, off=off, ids=ids, ex=exclusion_lists(dim, len(off) - 1, N_ITEM))


@functools.lru_cache(maxsize=None)
def wide_case():
    """BPR at dim 32 over 5000 POIs (an item range long enough to be cut into 64 slices) and 300 groups (above "group_split_max")."""
    C = make_case("bpr", 32, 341, n_user=N_USER, n_item=5000)
    rng = np.random.default_rng(342)
    groups = mixed_groups(343) + [rng.choice(N_USER, rng.integers(1, 7), replace=False) for _ in range(281)]
    off, ids = GO.csr(groups)
    return dict(C=C, sc=GO.member_scores(C["users"], C["items"]), off=off, ids=ids)


@functools.lru_cache(maxsize=None)
def tie_case():
    """BPR at dim 32 with POI 211 a copy of POI 57: equal scores for every member, hence for every group under both rules."""
    C = make_case("bpr", 32, 323, n_user=N_USER, n_item=300, twins=(57, 211))
    off, ids = GO.csr(mixed_groups(324))
    return dict(C=C, sc=GO.member_scores(C["users"], C["items"]), off=off, ids=ids, twins=(57, 211))


@functools.lru_cache(maxsize=None)
def tiny_case(n_item):
    """BPR at dim 8 over a table shorter than k: users / items (float64 views of float32 tables), the reference-layout tables, groups."""
    from tests.gpu_util import toy_problem
    T = toy_problem(70 + n_item, n_user=6, n_item=n_item, dim=8, hot=min(8, n_item - 1))
    rng = np.random.default_rng(71 + n_item)
    u32 = lambda *sh: np.float64(np.float32(rng.uniform(-0.5, 0.5, sh)))
    users, items = u32(6, 8), u32(n_item + 1, 8)
    off, ids = GO.csr([[0, 1, 2], [3], [4, 5, 0, 1], [], [2, 2]])
    ex = GO.csr([[], [0, 2], [], [], list(range(n_item))])
    return dict(T=T, users=users, items=items, sc=GO.member_scores(users, items), off=off, ids=ids, ex=ex)


def all_fixtures():
    """(name, member scores, off, ids, ex_off, ex, k) of every ranking fixture of the GPU tests."""
    for kind, dim in RANK_CASES:
        R = rank_case(kind, dim)
        yield "%s dim %d" % (kind, dim), R["sc"], R["off"], R["ids"], None, None, K
        yield "%s dim %d, lists" % (kind, dim), R["sc"], R["off"], R["ids"], R["ex"][0], R["ex"][1], K
    from poi_amd import data
    R = rank_case("bpr", 20)
    T = R["C"]["T"]
    xo, xi = data.group_exclusion_csr(*data.train_exclusion_csr(T["off"], T["p_flat"], T["n_item"]), R["off"], R["ids"], T["n_item"])
    yield "bpr dim 20, train lists", R["sc"], R["off"], R["ids"], xo, xi, K
    W = wide_case()
    yield "wide", W["sc"], W["off"], W["ids"], None, None, K
    for n_item in (13, 5):
        Y = tiny_case(n_item)
        yield "tiny %d" % n_item, Y["sc"], Y["off"], Y["ids"], Y["ex"][0], Y["ex"][1], K
    Tc = tie_case()
    yield "ties", Tc["sc"], Tc["off"], Tc["ids"], None, None, K
