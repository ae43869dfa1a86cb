"""-m gpu: the fused top-K scoring launches what its plan says (csrc/score_plan.h) - per case of tests/score_plan_cases.py the launch
counts of the timing regions - and every path returns the lists of the one-stage call (filter off, no seed), ids and score bits."""
import functools

import numpy as np
import pytest

from tests.score_plan_cases import CASES, K, REGIONS, SHORT_SEED_K

pytestmark = pytest.mark.gpu

DD = 200.0


@pytest.fixture(scope="module")
def pa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    poi_amd._lib.load()
    return poi_amd


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _problem(call, n, n_item, dim, n_dist):
    """Device operands of one (entry point, shape), shared by the cases on it, and the entry point as a function of (ctx, idx, sc)."""
    import torch
    from poi_amd.data import bin_thresholds, cos_lat
    import poi_amd
    ctx = poi_amd._lib.context(0)
    rng = np.random.default_rng(n * 7 + n_item + dim)
    du = _dev(rng.standard_normal((n, dim)).astype(np.float32))
    di = _dev(rng.standard_normal((n_item, dim)).astype(np.float32))
    keep = [du, di]
    if call in ("plain", "all"):
        def run(idx, sc):
            return ctx.lib.poi_score_topk(ctx.handle, du.data_ptr(), di.data_ptr(), n, n_item, dim, None, None, K, idx.data_ptr(), sc.data_ptr(), None)
        return run, keep
    n_pad = ((n + 31) // 32) * 32
    coords = np.stack([40.0 + 0.2 * rng.random(n_item), -74.0 + 0.2 * rng.random(n_item)], axis=1)
    sts = rng.random((n_pad, n_dist + 1)).astype(np.float32)
    sts[:, n_dist] = 0.0
    dwd, dsts = _dev(np.array([1.5], np.float32)), _dev(sts)
    dc, cph, thr = _dev(coords), _dev(cos_lat(coords)), _dev(bin_thresholds(DD, n_dist))
    dl = _dev(rng.integers(0, n_item, n).astype(np.int32))
    keep += [dwd, dsts, dc, cph, thr, dl]
    if call == "geo":
        def run(idx, sc):
            return ctx.lib.poi_score_topk_geo(ctx.handle, du.data_ptr(), di.data_ptr(), n, n_item, dim, dwd.data_ptr(), dsts.data_ptr(), dc.data_ptr(), cph.data_ptr(),
                                              thr.data_ptr(), dl.data_ptr(), n_dist, DD, K, idx.data_ptr(), sc.data_ptr(), None)
        return run, keep
    assert call == "bins8" and n_dist <= 255
    bins = torch.zeros((n_pad // 32) * ((n_item + 31) // 32) * 1024, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.poi_ulptai_build(ctx.handle, dc.data_ptr(), cph.data_ptr(), thr.data_ptr(), dl.data_ptr(), n, n_item, n_dist, DD, bins.data_ptr(), 1, None))
    keep.append(bins)

    def run(idx, sc):
        return ctx.lib.poi_score_topk_ulptai(ctx.handle, du.data_ptr(), di.data_ptr(), n, n_item, dim, dwd.data_ptr(), dsts.data_ptr(), bins.data_ptr(), 1, n_dist, K,
                                             idx.data_ptr(), sc.data_ptr(), None)
    return run, keep


def _lists(ctx, run, n, seed=None, filt=True, timed=False):
    """One call -> (ids, scores[, launches per region])."""
    import torch
    idx = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    sc = torch.zeros((n, K), dtype=torch.float32, device="cuda")
    try:
        ctx.set_topk_filter(filt)
        if seed is not None:
            ctx.set_topk_seed(seed, seed.shape[1])
        if timed:
            ctx.timing(True)
        ctx.check(run(idx, sc))
        torch.cuda.synchronize()
        counts = {r: ctx.timing_get(r)[1] for r in REGIONS} if timed else None
    finally:
        ctx.timing(False)
        ctx.set_topk_filter(True)
    return idx.cpu().numpy(), sc.cpu().numpy(), counts


@functools.lru_cache(maxsize=None)
def _one_stage(call, n, n_item, dim, n_dist):
    """The reference lists of a shape: the one-stage call, computed once."""
    import poi_amd
    run, _ = _problem(call, n, n_item, dim, n_dist)
    idx, sc, _ = _lists(poi_amd._lib.context(0), run, n, filt=False)
    assert (idx >= 0).all() and (idx < n_item).all() and (np.diff(sc, axis=1) <= 0).all()
    return idx, sc


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_call_launches_its_plan_and_returns_the_one_stage_lists(pa, case):
    import torch
    ctx = pa._lib.context(0)
    shape = (case["call"], case["n"], case["n_item"], case["dim"], case["n_dist"])
    n, n_item, dim = case["n"], case["n_item"], case["dim"]
    run, keep = _problem(*shape)
    eidx, esc = _one_stage(*shape)
    if case["call"] == "all":
        out = torch.zeros((n, n_item), dtype=torch.float32, device="cuda")
        ctx.timing(True)
        try:
            ctx.check(ctx.lib.poi_score_all(ctx.handle, keep[0].data_ptr(), keep[1].data_ptr(), n, n_item, dim, None, None, out.data_ptr(), None))
            torch.cuda.synchronize()
            counts = {r: ctx.timing_get(r)[1] for r in REGIONS}
        finally:
            ctx.timing(False)
        print(case["name"], counts)
        assert counts == case["counts"]
        # the matrix holds the lists' scores, bit for bit, at the lists' ids - and nothing larger
        S = out.cpu().numpy()
        assert np.array_equal(np.take_along_axis(S, eidx.astype(np.int64), axis=1).view(np.uint32), esc.view(np.uint32))
        assert np.array_equal(S.max(axis=1).view(np.uint32), esc[:, 0].view(np.uint32))
        return
    seed = {None: None, "true": eidx, "short": eidx[:, :SHORT_SEED_K]}[case["seed"]]
    idx, sc, counts = _lists(ctx, run, n, seed=None if seed is None else _dev(seed.astype(np.int32)), filt=case["filt"], timed=True)
    print(case["name"], counts)
    assert counts == case["counts"]
    assert np.array_equal(idx, eidx) and np.array_equal(sc.view(np.uint32), esc.view(np.uint32))
