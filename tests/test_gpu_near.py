"""-m gpu tests of the restricted recommendation (poi_score_topk_near -> models.compute_sub_topk_near, Session.recommend(within_km=,
exclude=), evaluate.device_rank_metrics(within_km=)): candidate sets, ranking, ties, exclusion, launch shapes, sessions, the contract
and the evaluation, all against the float64 oracle of tests/near_oracle.py run from the float32-rounded tables.  Problems come from the
generator of tests/test_gpu_session.py (a 40 km box)."""
import numpy as np
import pytest

from oracle import poi_oracle as O
from tests import near_oracle as NO
from tests.gpu_util import RTOL, round_f32
from tests.test_gpu_session import geo_problem, gru_init, oracle_rows, plain_model, seqs_of, spatial_init, spatial_model

pytestmark = pytest.mark.gpu

K = 20
AL = [0.01, 0.001]


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


# ---- cases: host-side tables and a builder for the model ---------------------------------------------------------------------------
def last_of(T):
    return T["train"][0][np.arange(T["n_user"]), T["lens"] - 1]


def make_case(kind, dim, seed, n_user=70, n_item=300, coords=None, twins=None, table_dtype="f32"):
    """dict(T, users, items (float64 views of the float32 tables, logical width), term, build(pa) -> model).  coords: replaces the
    generator's; twins (a, b): item row b is a copy of row a in every item table.  table_dtype="f16" (bpr / gru / spatial): the model
    stores its POI table as IEEE half, built from the same unrounded float32 `items` (tests/half_cases.py rounds them for the oracle)."""
    assert table_dtype == "f32" or kind in ("bpr", "gru", "spatial"), "%s stores float32 tables only" % kind
    kw = {} if table_dtype == "f32" else dict(table_dtype=table_dtype)
    T = geo_problem(seed, n_user=n_user, n_item=n_item, n_dist=11, dim=dim, len_min=4, len_max=8)
    if coords is not None:
        T["coords"] = coords
    rng = np.random.default_rng(seed + 7)
    u32 = lambda *s: np.float64(np.float32(rng.uniform(-0.5, 0.5, s)))
    users, term = u32(n_user, dim), None

    def twin(a):
        if twins is not None:
            a[twins[1]] = a[twins[0]]
        return a
    if kind in ("gru", "spatial"):
        P = gru_init(seed, T) if kind == "gru" else spatial_init(seed, T)
        P["lt"] = twin(P["lt"])
        items = P["lt"]
        if kind == "spatial":
            e = np.exp(rng.uniform(-2, 2, (n_user, T["n_dist"] + 1)))
            sts = np.float64(np.float32(e / e.sum(axis=1, keepdims=True)))
            term = (float(P["wd"]), sts)

        def build(pa):
            m = plain_model(pa, T, P, **kw) if kind == "gru" else spatial_model(pa, T, P, **kw)
            m.update_trained_users(users)
            if kind == "gru":
                m.set_coords(T["coords"])
            else:
                m.update_trained_sus(sts)
            return m
    elif kind == "bpr":
        items = twin(u32(n_item + 1, dim))

        def build(pa):
            m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=AL, n_user=n_user, n_item=n_item, n_in=dim, n_hidden=dim,
                                 init=dict(ux=users, lt=items), **kw)
            m.update_trained_items(); m.update_trained_users(); m.set_coords(T["coords"])
            return m
    elif kind == "vbpr":
        lt, ue, ei, fi = twin(u32(n_item + 1, dim)), u32(n_user, dim), u32(dim, 8), twin(u32(n_item + 1, 8))
        users, items = np.concatenate((users, ue), 1), np.concatenate((lt, fi @ ei.T), 1)

        def build(pa):
            m = pa.models.OboVBpr(train=T["train"], test=T["test"], alpha_lambda=AL + [0.001], n_user=n_user, n_item=n_item, n_in=dim, n_hidden=dim,
                                  n_img=8, fea_img=fi, init=dict(ux=users[:, :dim], lt=lt, ue=ue, ei=ei))
            m.update_trained_items(); m.update_trained_users(); m.set_coords(T["coords"])
            return m
    else:
        assert kind == "fpmc"
        ui, iu, ia, ai = u32(n_user, dim), twin(u32(n_item + 1, dim)), twin(u32(n_item + 1, dim)), u32(n_item + 1, dim)
        users, items = np.concatenate((ui, ai[last_of(T)]), 1), np.concatenate((iu, ia), 1)

        def build(pa):
            return pa.models.OboFpmc_lr(train=[[list(q) for q in seqs_of(T)], None, None], test=T["test"], alpha_lambda=AL, n_user=n_user,
                                        n_item=n_item, n_size=dim, coords=T["coords"], ud_km=8.0, init=dict(ui=ui, iu=iu, ia=ia, ai=ai))
    return dict(kind=kind, T=T, users=users, items=items, term=term, build=build)


def oracle_sc(C, anchor, items=None):
    T = C["T"]
    if C["term"] is None:
        return NO.scores(C["users"], C["items"] if items is None else items)
    return NO.scores(C["users"], C["items"], anchor, C["term"][0], C["term"][1], T["coords"], T["dd_m"], T["n_dist"])


def built(pa, C):
    """(model, oracle item table): VBPR's item table is formed on the device (poi_vbpr_items), so the oracle reads that float32 table."""
    m = C["build"](pa)
    items = np.float64(m.trained_items.get_value()) if C["kind"] == "vbpr" else None
    return m, items


def check(out, osc, mask, k, what, min_ok=0.9):
    """The whole ranking contract of one call: counts, exact lists on qualifying rows, and the every-row properties."""
    idx, sc, cnt = (t.cpu().numpy() for t in out)
    oid, oval, ocnt = NO.topk(osc, mask, k)
    assert idx.dtype == np.int32 and idx.shape == (len(osc), k) and np.array_equal(cnt, ocnt), what
    ok = NO.qualifying(osc, mask, k)
    print("%s: %.0f %% of %d rows qualify, candidates %d..%d" % (what, 100 * ok.mean(), len(ok), ocnt.min(), ocnt.max()))
    assert ok.mean() >= min_ok, "%s: only %.1f %% of the oracle's rows have clear gaps: pick another seed" % (what, 100 * ok.mean())
    assert np.array_equal(idx[ok], oid[ok]), what
    margin = RTOL * np.abs(osc).max()
    for r in range(len(osc)):
        m = min(k, int(ocnt[r]))
        g = idx[r, :m].astype(np.int64)
        assert np.all(idx[r, m:] == -1) and np.all(np.isneginf(sc[r, m:])), (what, r)
        assert len(set(g.tolist())) == m and g.min(initial=0) >= 0 and mask[r, g].all(), (what, r)
        assert m == 0 or np.abs(sc[r, :m] - osc[r, g]).max() <= margin, (what, r)
        rest = mask[r].copy(); rest[g] = False
        assert not (m and rest.any()) or osc[r, rest].max() <= osc[r, g].min() + margin, (what, r)
    return idx, sc, cnt


def near(m, rows, k=K, **kw):
    return m.compute_sub_topk_near(rows, k, return_scores=True, return_counts=True, **kw)


# ---- 1: candidate sets ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(pa):
    """BPR at dim 8 with two more POIs planted at the coordinates of user 0's last train POI."""
    T0 = geo_problem(11, n_user=70, n_item=300, n_dist=11, dim=8, len_min=4, len_max=8)
    a = int(last_of(T0)[0])
    co = [j for j in (41, 207, 133) if j != a][:2]
    xy = T0["coords"].copy(); xy[co] = xy[a]
    C = make_case("bpr", 8, 11, coords=xy)
    return C, C["build"](pa), a, co


@pytest.mark.parametrize("r_km", [0.0, 2.0, 8.0, 25.0, 1000.0])
def test_candidate_sets_are_exact_on_every_row(planted, r_km):
    C, m, a, co = planted
    T = C["T"]
    rows, anchor = np.arange(T["n_user"]), last_of(T)
    osc, mask = oracle_sc(C, anchor), NO.candidate_mask(T["coords"], anchor, r_km)
    idx, sc, cnt = check(near(m, rows, 32, within_km=r_km), osc, mask, 32, "radius %g km" % r_km)
    small = cnt <= 32
    assert small.any() or r_km >= 25
    for r in np.nonzero(small)[0]:
        assert set(idx[r, :cnt[r]].tolist()) == set(np.nonzero(mask[r])[0].tolist())
    if r_km == 0.0:      # the anchor and whatever shares its coordinates
        assert set(idx[0, :3].tolist()) == {a, *co} and cnt[0] == 3 and idx[0, 3] == -1
        lone = [r for r in rows if anchor[r] not in (a, *co)]
        assert np.array_equal(idx[lone, 0], anchor[lone]) and np.all(cnt[lone] == 1)
    if r_km == 1000.0:   # everything is inside: the unrestricted oracle top-K
        ok = NO.qualifying(osc, mask, 32)
        assert mask.all() and np.array_equal(idx[ok], O.topk_desc(osc, 32)[ok])


def test_fpmc_default_radius_is_the_neighbour_sets_plus_the_last_poi(pa):
    from poi_amd import data
    C = make_case("fpmc", 16, 14)
    T = C["T"]
    m = C["build"](pa)
    rows, anchor = np.arange(T["n_user"]), last_of(T)
    off, ids = data.fpmc_neighbors_host(T["coords"], m.ud_km)
    mask = np.zeros((T["n_user"], T["n_item"]), bool)
    for r, l in enumerate(anchor):
        mask[r, ids[off[l]:off[l + 1]]] = True; mask[r, l] = True
    assert np.array_equal(mask, NO.candidate_mask(T["coords"], anchor, m.ud_km))
    idx, sc, cnt = check(near(m, rows, 32), oracle_sc(C, anchor), mask, 32, "fpmc ud_km")
    small = cnt <= 32
    assert small.any()
    for r in np.nonzero(small)[0]:
        assert set(idx[r, :cnt[r]].tolist()) == set(np.nonzero(mask[r])[0].tolist())


# ---- 2: ranking ------------------------------------------------------------------------------------------------------------------------
RANK_CASES = [("bpr", 8), ("bpr", 20), ("bpr", 32), ("bpr", 128), ("bpr", 256), ("gru", 8), ("gru", 20), ("gru", 128), ("spatial", 32),
              ("spatial", 128), ("spatial", 256), ("vbpr", 16), ("vbpr", 64), ("fpmc", 16), ("fpmc", 128)]


@pytest.mark.parametrize("kind,dim", RANK_CASES)
def test_ranking_matches_the_oracle(pa, kind, dim):
    C = make_case(kind, dim, 100 + dim)
    T = C["T"]
    m, items = built(pa, C)
    assert m.kdim == {"bpr": dim, "gru": 64 if dim < 64 else dim, "spatial": 64 if dim < 64 else dim, "vbpr": 2 * dim, "fpmc": 2 * dim}[kind]
    rows, anchor = np.arange(T["n_user"]), last_of(T)
    osc = oracle_sc(C, anchor, items)
    for r_km in (8.0, 25.0):
        check(near(m, rows, within_km=r_km), osc, NO.candidate_mask(T["coords"], anchor, r_km), K, "%s dim %d, %g km" % (kind, dim, r_km))


# ---- 3: ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bpr", "spatial"])
def test_ties_come_out_in_ascending_id_order(pa, kind):
    """Two POIs with identical item rows at the same coordinates (the same bin): bitwise equal scores, the lower id first."""
    T0 = geo_problem(23, n_user=70, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    lo, hi = 57, 211
    xy = T0["coords"].copy(); xy[hi] = xy[lo]
    C = make_case(kind, 32, 23, coords=xy, twins=(lo, hi))
    T = C["T"]
    m, _ = built(pa, C)
    rows = np.arange(T["n_user"])
    anchor = np.full(T["n_user"], lo)                       # every row stands at the twins: both are candidates of every row
    osc, mask = oracle_sc(C, anchor), NO.candidate_mask(xy, anchor, 3.0)
    assert np.array_equal(osc[:, lo], osc[:, hi]) and mask.sum(axis=1).max() <= 32
    idx, sc, cnt = (t.cpu().numpy() for t in near(m, rows, 32, within_km=3.0, anchor=anchor))
    assert np.array_equal(cnt, mask.sum(axis=1))
    for r in rows:
        at = int(np.nonzero(idx[r] == lo)[0][0])
        assert idx[r, at + 1] == hi and sc[r, at] == sc[r, at + 1], r


# ---- 4: exclusion ----------------------------------------------------------------------------------------------------------------------
def test_exclusion_lists(pa):
    from poi_amd import data
    C = make_case("bpr", 32, 31)
    T = C["T"]
    m = C["build"](pa)
    rows, anchor = np.arange(T["n_user"]), last_of(T)
    osc = oracle_sc(C, anchor)
    lo_, li_ = data.last_exclusion_csr(anchor)
    to_, ti_ = data.train_exclusion_csr(T["off"], T["p_flat"], T["n_item"])
    rng = np.random.default_rng(5)
    lists = [np.sort(rng.choice(T["n_item"], rng.integers(0, 40), replace=False)) for _ in rows]
    lists[3] = np.arange(T["n_item"])                       # removes every candidate of row 3
    xo, xi = np.r_[0, np.cumsum([len(l) for l in lists])], np.concatenate(lists)
    for name, arg, eo, ei, r_km in (("last", "last", lo_, li_, 8.0), ("train", "train", to_, ti_, 8.0), ("csr", (xo, xi), xo, xi, 8.0),
                                    ("csr, no radius", (xo, xi), xo, xi, None), ("last at 0 km", "last", lo_, li_, 0.0),
                                    ("train at 2 km", "train", to_, ti_, 2.0)):
        mask = NO.candidate_mask(T["coords"], anchor, r_km, eo, ei)
        idx, sc, cnt = check(near(m, rows, within_km=r_km, exclude=arg), osc, mask, K, "exclude " + name)
        if name.startswith("csr"):
            assert cnt[3] == 0 and np.all(idx[3] == -1) and np.all(np.isneginf(sc[3]))
        if name == "last at 0 km":                           # nothing shares an anchor's coordinates: every list is empty
            assert np.all(cnt == 0) and np.all(idx == -1)
        if name == "train at 2 km":
            assert ((cnt > 0) & (cnt < K)).any(), "no row with a -1 tail"
    # "train" on an id list that is no contiguous range gathers the cached lists
    sub = np.array([9, 3, 60, 17, 3])
    mask = NO.candidate_mask(T["coords"], anchor[sub], 8.0, *data.train_exclusion_csr(
        np.r_[0, np.cumsum(T["lens"][sub])], np.concatenate([seqs_of(T)[u] for u in sub]), T["n_item"]))
    check(near(m, sub, within_km=8.0, exclude="train"), osc[sub], mask, K, "exclude train, gathered rows", min_ok=0.0)


# ---- 5: launch shapes ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(pa):
    """5000 POIs and an all-covering radius: a band long enough to be split over workgroups and merged."""
    C = make_case("bpr", 32, 41, n_user=70, n_item=5000)
    T = C["T"]
    anchor = last_of(T)
    return C, C["build"](pa), anchor, oracle_sc(C, anchor), NO.candidate_mask(T["coords"], anchor, 1000.0, *pa.data.last_exclusion_csr(anchor))


@pytest.mark.parametrize("n", [1, 33, 70])
def test_launch_shapes_and_both_paths(wide, n):
    import torch
    C, m, anchor, osc, mask = wide
    rows = np.arange(70 - n, 70)
    default = 256
    ref = None
    try:
        for split_max, grid in ((None, 0), (0, 0), (1 << 30, 1), (1 << 30, 2), (1 << 30, 7), (1 << 30, 64)):
            if split_max is not None:
                m.ctx.set_option("near_split_max", split_max)
            m.ctx.set_option("near_grid", grid)
            out = near(m, rows, within_km=1000.0, exclude="last")
            plan = {k: m.ctx.last_plan(k) for k in ("near_path", "near_splits", "near_split_max")}
            if split_max is None:
                assert plan["near_split_max"] == default and plan["near_path"] == 1 and 2 <= plan["near_splits"] <= 64, plan
            elif split_max == 0:
                assert plan == dict(near_path=0, near_splits=0, near_split_max=0), plan
            else:
                assert plan == dict(near_path=1, near_splits=grid, near_split_max=1 << 30), plan
            check(out, osc[rows], mask[rows], K, "n %d split_max %r grid %d" % (n, split_max, grid))
            again = near(m, rows, within_km=1000.0, exclude="last")
            assert all(torch.equal(a, b) for a, b in zip(out, again)), "two identical calls differ"
            ref = ref or out
            assert all(torch.equal(a, b) for a, b in zip(out, ref)), "two grids differ"
    finally:
        m.ctx.set_option("near_split_max", default); m.ctx.set_option("near_grid", 0)


def test_defaults_are_compute_sub_topk(wide):
    import torch
    C, m, anchor, osc, mask = wide
    rows = np.arange(5, 41)
    a, b = m.compute_sub_topk_near(rows, K, return_scores=True), m.compute_sub_topk(rows, K, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and an infinite radius through the restricted kernel ranks the same POIs
    idx, sc, cnt = check(near(m, rows, within_km=float("inf"), anchor=anchor[rows]), osc[rows], np.ones_like(mask[rows]), K, "no radius")
    assert np.all(cnt == C["T"]["n_item"])


# ---- 6: sessions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [True, False])
def test_session_recommend_restricted(pa, spatial):
    import torch
    T = geo_problem(60, n_user=64, n_item=300, n_dist=11, dim=32, len_min=4, len_max=8)
    P = spatial_init(32, T) if spatial else gru_init(32, T)
    m = spatial_model(pa, T, P) if spatial else plain_model(pa, T, P)
    if not spatial:
        with pytest.raises(pa._lib.PoiError, match="set_coords"):
            m.session().recommend([0], K, within_km=5)
        m.set_coords(T["coords"])
    s = m.session(n_slot=T["n_user"] + 2)
    s.replay(T["off"], T["p_flat"])
    slots = np.arange(T["n_user"] + 2)                      # the last two never checked in
    plain = s.recommend(slots, K, return_scores=True)
    hts, sts = oracle_rows(P, T, seqs_of(T), spatial=spatial)
    users = np.concatenate((hts, np.zeros((2, T["dim"]))))
    anchor = np.r_[last_of(T), -1, -1]
    if spatial:
        osc = NO.scores(users, P["lt"], anchor, P["wd"], np.concatenate((sts, np.zeros((2, sts.shape[1])))), T["coords"], T["dd_m"], T["n_dist"])
    else:
        osc = NO.scores(users, P["lt"])
    mask = NO.candidate_mask(T["coords"], anchor, 5.0, *pa.data.last_exclusion_csr(anchor))
    idx, sc, cnt = check(s.recommend(slots, K, return_scores=True, within_km=5, exclude="last", return_counts=True), osc, mask, K,
                         "session spatial=%s" % spatial, min_ok=0.0)
    ok = NO.qualifying(osc[:-2], mask[:-2], K)
    assert ok.mean() >= 0.9
    # no check-in: the radius is ignored, no distance term - 0 . items, all ties, ascending id
    assert np.all(cnt[-2:] == T["n_item"]) and np.array_equal(idx[-2:], np.tile(np.arange(K), (2, 1))) and np.all(sc[-2:] == 0.0)
    # the default arguments keep today's path, bit for bit
    again = s.recommend(slots, K, return_scores=True, within_km=None, exclude=None, return_counts=False)
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])
    with pytest.raises(ValueError):
        s.recommend(slots, K, exclude="train")


# ---- 7: contract -----------------------------------------------------------------------------------------------------------------------
def test_contract(pa, planted):
    import torch
    C, m, a, co = planted
    T = C["T"]
    rows, anchor = np.arange(8), last_of(T)[:8].copy()
    osc = oracle_sc(C, last_of(T))[:8]
    dev = lambda v: torch.as_tensor(np.asarray(v, np.int32)).to(m.device)
    for bad_value in (T["n_item"], -2):
        bad = anchor.copy(); bad[2] = bad_value
        with pytest.raises(IndexError):                      # a host array: refused before any launch
            near(m, rows, within_km=8.0, anchor=bad)
        assert m.ctx.take_bad_ids() == 0
        with pytest.raises(IndexError):                      # a device tensor: the kernel counts the row
            near(m, rows, within_km=8.0, anchor=dev(bad))
        idx, sc, cnt = (t.cpu().numpy() for t in near(m, rows, within_km=8.0, anchor=dev(bad), sync=False))
        assert m.ctx.take_bad_ids() == 1
        assert np.all(idx[2] == -1) and np.all(np.isneginf(sc[2])) and cnt[2] == 0
        good = np.arange(8) != 2
        mask = NO.candidate_mask(T["coords"], anchor, 8.0)
        check(tuple(torch.as_tensor(v[good]) for v in (idx, sc, cnt)), osc[good], mask[good], K, "rows beside a bad anchor", min_ok=0.0)
    # a device exclusion list with an id out of range is a bad row too
    eo, ei = dev(np.arange(9)), dev([1, 2, 3, T["n_item"], 5, 6, 7, 8])
    idx = m.compute_sub_topk_near(rows, K, within_km=8.0, exclude=(eo, ei), sync=False).cpu().numpy()
    assert m.ctx.take_bad_ids() == 1 and np.all(idx[3] == -1) and idx[4, 0] >= 0
    for off, ids, exc in (([0, 1, 2, 3, 4, 5, 6, 7, 9], [1, 2, 3, 4, 5, 6, 7, 9, 8], ValueError), ([0] * 8 + [1], [T["n_item"]], IndexError),
                          ([0] * 8, [], ValueError)):
        with pytest.raises(exc):
            m.compute_sub_topk_near(rows, K, within_km=8.0, exclude=(off, ids))
    with pytest.raises(pa._lib.PoiError, match="k <= 32"):
        m.compute_sub_topk_near(rows, 33, within_km=8.0)
    with pytest.raises(ValueError):
        m.compute_sub_topk_near(rows, K, within_km=-1.0)
    # no coordinates yet
    bare = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=AL, n_user=T["n_user"], n_item=T["n_item"], n_in=8, n_hidden=8)
    with pytest.raises(pa._lib.PoiError, match="set_coords"):
        bare.compute_sub_topk_near(rows, K, within_km=8.0)
    assert bare.compute_sub_topk_near(rows, K, exclude="train").shape == (8, K)      # no radius: no coordinates needed


def test_models_with_their_own_score_rule_raise(pa):
    M = pa.models
    for cls in (M.OboCARNN, M.OboPrme, M.OboPRPRM, M.OboGeoIE, M.OboPoi2vec):
        obj = cls.__new__(cls)                               # the refusal comes before anything of the model is read
        with pytest.raises(pa._lib.PoiError, match="score rule of its own"):
            obj.compute_sub_topk_near([0], K, within_km=5.0)


# ---- 8: evaluation ---------------------------------------------------------------------------------------------------------------------
def test_device_rank_metrics_restricted(pa):
    from poi_amd import evaluate
    C = make_case("bpr", 32, 52)
    T = C["T"]
    m = C["build"](pa)
    rows, anchor = np.arange(T["n_user"]), last_of(T)
    osc = oracle_sc(C, anchor)
    at = [5, 10, 20]
    for r_km, ex, lists in ((6.0, None, (None, None)), (25.0, "train", pa.data.train_exclusion_csr(T["off"], T["p_flat"], T["n_item"]))):
        mask = NO.candidate_mask(T["coords"], anchor, r_km, *lists)
        assert NO.qualifying(osc, mask, at[-1]).all(), "every row must qualify: pick another seed"
        oid, _, ocnt = NO.topk(osc, mask, at[-1])
        assert r_km > 10 or (ocnt < at[-1]).any(), "no row with -1 ids"
        exp = evaluate.rank_metrics(oid, T["test"][0], T["test"][1], at)
        got = evaluate.device_rank_metrics(m, [rows[:32], rows[32:]], at, within_km=r_km, exclude=ex)
        for k in at:
            for key in ("hits", "recall", "precision", "f1", "map", "ndcg"):
                assert abs(got[k][key] - exp[k][key]) <= 1e-12 * max(1.0, abs(exp[k][key])), (r_km, k, key, got[k][key], exp[k][key])
    # the defaults are the unrestricted evaluation
    assert evaluate.device_rank_metrics(m, [rows], at) == evaluate.device_rank_metrics(m, [rows], at, within_km=None, exclude=None)
