"""-m gpu: a rejected element must equal its removal, on every sort-based training step (csrc/bpr.hip, fpmc.hip, prme.hip, vbpr.hip,
geoie.hip, poi2vec.hip) at the placements of tests/reject_cases.py: the sentinel run starting on a 64-touch window boundary, a sentinel run
longer than a window, launches that are all sentinel (n = 1 included), a rejected element that is the only toucher of a row, every id bad,
every rejection kind.  Per case and cap:
  1. every table within assert_step_close (RTOL, DELTA_RTOL) of the step's float64 oracle batch rule on the KEPT elements, kept losses
     within assert_close (a half POI table of BPR: the one-ulp comparison of test_gpu_bpr.test_bpr_snapshot_half_poi_table);
  2. every table and kept loss bitwise equal to the same launch WITHOUT the rejected elements;
  3. rejected losses NaN, poi_ctx_take_bad_ids == the number of rejected elements, a second read 0;
  4. reserved rows, and every row no kept element names, bit-equal to their entry values.
The launchers and oracles are the per-step tests' own.  tests/test_reject_cases_cpu.py shows that the BPR fixtures separate the clamped-key
rule csrc/bpr.hip had before from this contract by >= 10x the update bar."""
import numpy as np
import pytest
import torch

from oracle import poi_oracle as O
from tests import fpmc_oracle as FO, geoie_oracle as GO, poi2vec_oracle as PO2, prme_oracle as PO, reject_cases as RC, vbpr_oracle as V
from tests import test_gpu_fpmc as TF, test_gpu_geoie as TG, test_gpu_poi2vec as TP2, test_gpu_prme as TP, test_gpu_vbpr as TV
from tests.gpu_util import assert_close, assert_step_close, round_f32, toy_problem
from tests.test_gpu_bpr import _expected_vec

pytestmark = pytest.mark.gpu

ALPHA, LAM = 0.01, 0.001
NU, NI = RC.N_USER, RC.N_ITEM
CAPS = [1.0, 8.0, 1e9]
CASES = {s: RC.build(s) for s in RC.SPECS}
HOGWILD = RC.build("bpr", disjoint=True)


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available()
    import poi_amd
    return poi_amd


@pytest.fixture(scope="module")
def ctx():
    from poi_amd import _lib
    return _lib.context(0)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _f64(T, names):
    return {k: T[k].float().cpu().numpy().astype(np.float64) for k in names}


def _check(c, step, names, rows_of, entry, full, removed, exp, exp_loss, what, oracle_check=None):
    """entry / full[0] / removed[0]: {table: device tensor}; full, removed = (tables, losses, bad count, second read); exp: oracle tables
    from the kept elements; rows_of: {table: id fields naming its rows} (tables without an entry are dense)."""
    T, loss, bad, again = full
    n_rej = len(c.rejected)
    # 3. losses and counts
    assert np.isnan(loss[c.rejected]).all(), what
    assert np.isfinite(loss[c.keep]).all(), what
    assert bad == n_rej and again == 0, (what, bad, again, n_rej)
    # 1. the oracle on the kept elements
    if oracle_check is None:
        if len(c.keep):
            assert_close(loss[c.keep], exp_loss, "kept losses " + what)
        P = _f64(entry, names)
        worst = assert_step_close(_f64(T, names), exp, P, names, what)
        print("%s: worst weight error %.3g" % (what, worst))
    else:
        oracle_check()
    # 2. the launch without the rejected elements
    if removed is not None:
        T2, loss2, bad2, _ = removed
        assert bad2 == 0
        for k in names:
            assert torch.equal(_bits(T[k]), _bits(T2[k])), (what, k, "differs from the launch without the rejected elements")
        assert np.array_equal(loss[c.keep].view(np.uint32), loss2.view(np.uint32)), what
    else:
        for k in names:
            assert torch.equal(_bits(T[k]), _bits(entry[k])), (what, k, "moved in a launch that is all rejected")
    # 4. reserved rows and rows no kept element names
    for k, fields in rows_of.items():
        named = np.unique(np.concatenate([c.launch[f][c.keep] for f in fields])) if len(c.keep) else np.zeros(0, np.int64)
        res = c.res_user if fields == (RC.SPECS[step].user,) else c.res_poi
        assert not np.intersect1d(named, res).size
        free = torch.as_tensor(np.setdiff1d(np.arange(T[k].shape[0]), named)).to(T[k].device)
        assert torch.equal(_bits(T[k])[free], _bits(entry[k])[free]), (what, k, "a row no kept element names moved")
        r = torch.as_tensor(res).to(T[k].device)
        assert torch.equal(_bits(T[k])[r], _bits(entry[k])[r]), (what, k, "a reserved row moved")


# ---- BPR ----------------------------------------------------------------------------------------------------------------------------
_TOY = {}


def _bpr_run(pa, P, dim, L, cap, table, mode="snapshot"):
    T = _TOY.setdefault(dim, toy_problem(3, n_user=NU, n_item=NI, dim=dim))
    m = pa.models.OboBpr(train=T["train"], test=T["test"], alpha_lambda=[ALPHA, LAM], n_user=NU, n_item=NI, n_in=dim, n_hidden=dim, init=P,
                         table_dtype="f32" if table == "f32" else "f16")
    entry = {"ux": m.ux.t.clone(), "lt": m.lt.t.clone()}
    m.ctx.take_bad_ids()
    m.ctx.set_batch_cap(cap)
    if table != "f32":
        m.ctx.set_f16_rounding(table, seed=3)          # (the same salt for the launch with and the launch without)
    try:
        loss = m.train_batch(L["u"], L["p"], L["q"], mode=mode, sync=False)
        bad = m.ctx.take_bad_ids()
        again = m.ctx.take_bad_ids()
    finally:
        m.ctx.set_batch_cap(1.0); m.ctx.set_f16_rounding("nearest", seed=1)
    return entry, ({"ux": m.ux.t.clone(), "lt": m.lt.t.clone()}, loss.cpu().numpy(), bad, again), m


def _bpr_case(pa, c, dim, cap, table, mode="snapshot"):
    P = round_f32(O.init_bpr_params(np.random.default_rng(70 + dim), NU, NI, dim))
    if table != "f32":
        P["lt"] = np.asarray(P["lt"], np.float16).astype(np.float64)      # the stored values ARE halves
    what = "bpr %s %s dim %d cap %g %s" % (mode, c.name, dim, cap, table)
    entry, full, m = _bpr_run(pa, P, dim, c.launch, cap, table, mode)
    removed = _bpr_run(pa, P, dim, RC.take(c.launch, c.keep), cap, table, mode)[1] if len(c.keep) else None
    u, p, q = (c.launch[f][c.keep] for f in "upq")
    exp, el = _expected_vec(P, u, p, q, ALPHA, LAM, cap)
    oracle_check = None
    if table != "f32":
        def oracle_check():
            if len(c.keep):
                assert_close(full[1][c.keep], el, "kept losses " + what)
            assert_close(m.ux.get_value(), exp["ux"], "ux " + what)
            lt = m.lt.get_value().astype(np.float64)
            want = np.asarray(exp["lt"], np.float16).astype(np.float64)
            ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
            assert (np.abs(lt - want) <= ulp).all(), what
    else:
        got = {k: getattr(m, k).get_value() for k in ("ux", "lt")}      # (logical shapes)
        def oracle_check():
            if len(c.keep):
                assert_close(full[1][c.keep], el, "kept losses " + what)
            print("%s: worst weight error %.3g" % (what, assert_step_close(got, exp, P, ("ux", "lt"), what)))
    _check(c, "bpr", ("ux", "lt"), {"ux": ("u",), "lt": ("p", "q")}, entry, full, removed, exp, el, what, oracle_check)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dim,table", [(20, "f32"), (64, "f32"), (64, "nearest"), (64, "stochastic")])
@pytest.mark.parametrize("name", list(CASES["bpr"]))
def test_bpr_snapshot(pa, name, dim, table, cap):
    _bpr_case(pa, CASES["bpr"][name], dim, cap, table)


@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", list(HOGWILD))
def test_bpr_hogwild_on_disjoint_rows(pa, name, dim):
    """the kept triples share no row: the racy kernel is the reference; one count per rejected triple, as in snapshot mode"""
    _bpr_case(pa, HOGWILD[name], dim, 1.0, "f32", mode="hogwild")


# ---- FPMC-LR, PRME: raw launches ----------------------------------------------------------------------------------------------------
def _raw_run(ctx, mod, P, dim, args, cap):
    T = mod._tables(P)
    ctx.take_bad_ids()
    ctx.set_batch_cap(cap)
    try:
        loss = mod._launch(ctx, T, NU, NI, dim, *args)
        bad = ctx.take_bad_ids()
        again = ctx.take_bad_ids()
    finally:
        ctx.set_batch_cap(1)
    return T, loss, bad, again


def _raw_case(ctx, step, mod, orc, fields, rows_of, c, dim, cap):
    T0 = mod._tables(orc.init_tables(np.random.default_rng(80 + dim), NU, NI, dim))
    P = mod._host(T0)                                                       # float32-rounded entry values
    what = "%s %s dim %d cap %g" % (step, c.name, dim, cap)
    args = lambda L: [L[f] for f in fields]
    full = _raw_run(ctx, mod, P, dim, args(c.launch), cap)
    kept = RC.take(c.launch, c.keep)
    removed = _raw_run(ctx, mod, P, dim, args(kept), cap) if len(c.keep) else None
    exp, el = orc.batch_step(P, *args(kept), ALPHA, LAM, cap=cap)
    _check(c, step, orc.TABLES, rows_of, T0, full, removed, exp, el, what)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", list(CASES["fpmc"]))
def test_fpmc(ctx, name, dim, cap):
    _raw_case(ctx, "fpmc", TF, FO, ("u", "a", "i", "j"), {"ui": ("u",), "ai": ("a",), "iu": ("i", "j"), "ia": ("i", "j")},
              CASES["fpmc"][name], dim, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", list(CASES["prme"]))
def test_prme(ctx, name, dim, cap):
    _raw_case(ctx, "prme", TP, PO, ("u", "p", "q", "prev", "d", "gap"), {"du": ("u",), "dp": ("p", "q", "prev"), "ds": ("p", "q", "prev")},
              CASES["prme"][name], dim, cap)


# ---- VBPR ---------------------------------------------------------------------------------------------------------------------------
_VSET = {}


def _vbpr_run(pa, T, P, fi, D, F, L, cap):
    m = TV._model(pa, T, P, fi, D, F)
    entry = {k: getattr(m, k).t.clone() for k in V.NAMES}
    m.ctx.take_bad_ids()
    m.ctx.set_batch_cap(cap)
    try:
        loss = m.train_batch(L["u"], L["p"], L["q"], sync=False).cpu().numpy()
        bad = m.ctx.take_bad_ids()
        again = m.ctx.take_bad_ids()
    finally:
        m.ctx.set_batch_cap(1.0)
    assert np.array_equal(m.fi.get_value(), fi.astype(np.float32))
    return entry, ({k: getattr(m, k).t.clone() for k in V.NAMES}, loss, bad, again)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("D,F", [(20, 100), (64, 1024)])
@pytest.mark.parametrize("name", list(CASES["vbpr"]))
def test_vbpr(pa, name, D, F, cap):
    """(every launch here is far below 4096 triples, where the dense ei gradient's chunking does not depend on the launch size)"""
    c = CASES["vbpr"][name]
    if D not in _VSET:
        _VSET[D] = TV._setup(pa, 52, NU, NI, D, F, "scaled")
    T, P, fi = _VSET[D]
    what = "vbpr %s D %d F %d cap %g" % (c.name, D, F, cap)
    entry, full = _vbpr_run(pa, T, P, fi, D, F, c.launch, cap)
    kept = RC.take(c.launch, c.keep)
    removed = _vbpr_run(pa, T, P, fi, D, F, kept, cap)[1] if len(c.keep) else None
    exp, el = V.batch_step(P, fi, kept["u"], kept["p"], kept["q"], ALPHA, LAM, TV.LAM_EV, cap)
    _check(c, "vbpr", V.NAMES, {"ux": ("u",), "ue": ("u",), "lt": ("p", "q")}, entry, full, removed, exp, el, what)


# ---- GeoIE, POI2Vec: whole users are rejected ---------------------------------------------------------------------------------------
_GEO = {}
GEO_GOOD = list(range(14))
GEO_BAD = {"p_high": 14, "q_neg": 15, "user_high": 18, "user_neg": -1}      # users 16, 17: never launched


def _geoie_problem(dim):
    """18 users over 120 POIs: users 0 .. 13 (histories of 0 .. 30, one of 0 and one of 1: no rows, loss 0, not a rejection) name POIs < 100
    only; users 14 and 15 name the reserved POIs 100 .. 119 only and have one id outside the table (SOLE TOUCHERS of those rows)."""
    if dim not in _GEO:
        lens = [6, 9, 30, 12, 0, 20, 8, 15, 1, 2, 3, 25, 17, 5, 12, 11, 4, 4]
        P, seqs, coords = TG._problem(21 + dim, len(lens), 120, dim, lens, revisit=0.3, b=0.2)
        seqs = [(np.asarray(p) % 100, np.asarray(q) % 100) for p, q in seqs]
        rng = np.random.default_rng(5)
        for u, (field, at, val) in ((14, (0, 3, 121)), (15, (1, 5, -2))):
            L = lens[u]
            pq = [100 + rng.permutation(10)[:L] if L <= 10 else 100 + rng.permutation(20)[:L], 100 + rng.integers(0, 20, L)]
            pq[field][at] = val
            seqs[u] = (pq[0], pq[1])
        _GEO[dim] = (P, seqs, coords, RC.user_cases(GEO_GOOD, GEO_BAD))
    return _GEO[dim]


GEO_NAMES = list(RC.user_cases(GEO_GOOD, GEO_BAD))


@pytest.mark.parametrize("cap", [1.0, 64.0, 1e9])
@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", GEO_NAMES)
def test_geoie(ctx, name, dim, cap):
    P, seqs, coords, cases = _geoie_problem(dim)
    c = cases[name]
    what = "geoie %s dim %d cap %g" % (name, dim, cap)

    def run(users):
        X = TG.Launch(P, seqs, coords)
        ctx.take_bad_ids()
        ctx.set_batch_cap(cap)
        try:
            loss = X.step(ctx, users)
            bad, again = ctx.take_bad_ids(), ctx.take_bad_ids()
        finally:
            ctx.set_batch_cap(1)
        return X, loss, bad, again
    X, loss, bad, again = run(c.users)
    assert np.isnan(loss[c.rejected]).all() and np.isfinite(loss[c.keep]).all(), what
    assert bad == len(c.rejected) and again == 0, (what, bad, again)
    E = TG.Launch(P, seqs, coords)                                             # entry values
    if len(c.keep):
        kept = c.users[c.keep]
        Q, ref, M = GO.batch_step(P, [seqs[u] for u in kept], coords, ALPHA, LAM, cap=cap, absmass=True)
        assert_close(loss[c.keep], ref, "kept losses " + what)
        TG._check_step(X.host(), Q, P, what, absmass=M)
        Y, loss2, bad2, _ = run(kept)
        assert bad2 == 0 and np.array_equal(loss[c.keep].view(np.uint32), loss2.view(np.uint32)), what
        named = np.unique(np.concatenate([np.concatenate(seqs[u]) for u in kept]))
    else:
        Y, named = E, np.zeros(0, np.int64)
    for t in GO.TABLES:
        assert torch.equal(_bits(X.T[t]), _bits(Y.T[t])), (what, t, "differs from the launch without the rejected users")
    assert torch.equal(X.ab.view(torch.int64), Y.ab.view(torch.int64)), what
    assert named.size == 0 or named.max() < 100
    free = torch.as_tensor(np.setdiff1d(np.arange(121), named)).cuda()         # the reserved rows 100 .. 120 among them
    for t in ("g", "h", "z"):
        assert torch.equal(_bits(X.T[t])[free], _bits(E.T[t])[free]), (what, t, "a row no kept user names moved")
    assert torch.equal(_bits(X.T["t"]), _bits(E.T["t"]))


_P2V = {}
P2V_LENS = [5, 0, 9, 3, 14, 6, 2, 11, 30, 1, 7, 4, 12, 8, 20, 3]
P2V_GOOD = [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
P2V_BAD = {"empty": 1, "target": 3, "user_high": len(P2V_LENS), "user_neg": -1}
P2V_NAMES = list(RC.user_cases(P2V_GOOD, P2V_BAD))


@pytest.mark.parametrize("cap", [1, 64, 1e9])
@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", P2V_NAMES)
def test_poi2vec(ctx, name, dim, cap):
    """user 1 has no train target, user 3 a target outside the table (written into the device copy of the targets), two ids are outside
    the user table.  wl is touched by every accepted user (the full softmax): only xu has rows no kept user names."""
    if dim not in _P2V:
        _P2V[dim] = TP2.problem(61 + dim, 120, dim, P2V_LENS)
    pr = _P2V[dim]
    c = RC.user_cases(P2V_GOOD, P2V_BAD)[name]
    what = "poi2vec %s dim %d cap %g" % (name, dim, cap)

    def run(users):
        m = TP2.model_of(pr)
        m.tgt[int(m._tra[0][3]) + 1] = 120 + 3
        entry = {"xu": m._xu.clone(), "wl": m._wl.clone(), "pb": m._pb.clone()}
        ctx.take_bad_ids()
        ctx.set_batch_cap(cap)
        try:
            loss = TP2._raw_step(ctx, m, users)
            bad, again = ctx.take_bad_ids() + m.rejected, ctx.take_bad_ids()
        finally:
            ctx.set_batch_cap(1)
        return m, entry, loss, bad, again
    m, entry, loss, bad, again = run(c.users)
    now = {"xu": m._xu, "wl": m._wl, "pb": m._pb}
    assert np.isnan(loss[c.rejected]).all() and np.isfinite(loss[c.keep]).all(), what
    assert bad == len(c.rejected) and again == 0, (what, bad, again)
    if len(c.keep):
        kept = c.users[c.keep]
        Q, ref, M = PO2.batch_step(pr["P"], pr["T"], kept, pr["data"], ALPHA, LAM, pr["len_max"], cap=cap, absmass=True)
        assert_close(loss[c.keep], ref, "kept losses " + what)
        assert_step_close(TP2.tables(m), Q, pr["P"], TP2.TABLES, what, absmass=M)
        m2, _, loss2, bad2, _ = run(kept)
        assert bad2 == 0 and np.array_equal(loss[c.keep].view(np.uint32), loss2.view(np.uint32)), what
        other = {"xu": m2._xu, "wl": m2._wl, "pb": m2._pb}
        named = np.unique(kept)
    else:
        other, named = entry, np.zeros(0, np.int64)
    for k in now:
        assert torch.equal(_bits(now[k]), _bits(other[k])), (what, k, "differs from the launch without the rejected users")
    free = torch.as_tensor(np.setdiff1d(np.arange(len(P2V_LENS)), named)).cuda()      # the rejected users' own rows among them
    assert torch.equal(_bits(now["xu"])[free], _bits(entry["xu"])[free]), (what, "an xu row no kept user names moved")
