"""Static guard on the hybrid recurrences' reproducibility (abi.hip, TeArgs.hyb): at dim 128 the launches of 1150 .. 2300 sequences run
the leading sequences on the per-sequence kernels (te_rec_fwd1x / te_rec_bwd1, stream side2) WHILE the rest runs in 16-sequence tiles
(te_rec_fwdx / te_rec_bwd16t).  Identical launches are bitwise identical only because a workgroup of the per-sequence kernel can never
be resident on a CU together with a workgroup of the tile kernel (abi.hip at the `A.hyb` predicate, docs/NOTEBOOK.md: at dim 64, where
they do fit one CU, identical launches differed in the last bits of DA).  This test reads the registers and LDS of the exact template
instances from the library's gfx950 code objects (tools/scan_waits.py, as tests/test_static_scan.py does) and checks that budget
against the capacity of one CU:
  * 4 SIMDs, each with 512 VGPR + AGPR per lane for all its waves, allocated in granules of 8 registers;
  * a workgroup of T threads puts ceil(T / 64 / 4) waves on each SIMD (512 threads: 2 waves per SIMD), at most 8 waves per SIMD;
  * 160 KiB of LDS per CU (static LDS from the code object + the dynamic LDS of the launch).
The metadata's .vgpr_count is the unified count on gfx950 (arch VGPRs rounded up to 4, plus the AGPRs): taking it as the whole
allocation can only UNDER-state a wave's registers, so "does not fit" stays a safe conclusion.  Skipped when the ROCm binary tools
are not installed."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc")
spec = importlib.util.spec_from_file_location("scan_waits", os.path.join(ROOT, "tools", "scan_waits.py"))
scan_waits = importlib.util.module_from_spec(spec)
spec.loader.exec_module(scan_waits)

SIMDS, REGS_PER_SIMD, GRANULE, WAVES_PER_SIMD, LDS_PER_CU = 4, 512, 8, 8, 160 * 1024
XS = 5            # te_xfwd.hip: signed base-256 digits per operand (pinned below)


def fwdx_dyn_lds(D):
    """te_xfwd.hip te_xfwd_lds(D): the dynamic LDS of te_rec_fwdx<D, FT, false> (XRec<D>::lds())."""
    KB, NW, SL = D // 64, D // 16, XS - 3
    return 2 * XS * 16 * (D + 16) + NW * 3 * KB * SL * 64 * 16


def bwd16t_dyn_lds(D):
    """tile_engine.hip launch_te_train: sizeof(short) * (3 * 16 * (3 * D + 16) + 3 * D * D)."""
    return 2 * (3 * 16 * (3 * D + 16) + 3 * D * D)


# (per-sequence kernel, its dynamic LDS), (tile kernel, its dynamic LDS): the pairs the hybrid runs at the same time; FT = the forward
# table variant (TeArgs.xft).  Block size 4 D for all four (pinned below).
def pairs(D):
    return [(("te_rec_fwd1x_kernel<%d, false, %s>" % (D, ft), 0), ("te_rec_fwdx_kernel<%d, %s, false>" % (D, ft), fwdx_dyn_lds(D)))
            for ft in ("false", "true")] + \
           [(("te_rec_bwd1_kernel<%d>" % D, 0), ("te_rec_bwd16t_kernel<%d>" % D, bwd16t_dyn_lds(D)))]


NAMES = sorted({k for D in (64, 128) for p in pairs(D) for k, _ in p})


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import poi_amd
    poi_amd.build.build_lib()                      # (no-op when the library is up to date)
    if not scan_waits.available():
        pytest.skip("llvm-objdump / clang-offload-bundler not installed")
    recs = scan_waits.scan(NAMES, tmp=str(tmp_path_factory.mktemp("scan")))
    return {r["kernel"]: r for r in recs if "loop" not in r}


def per_simd_regs(r, threads):
    waves = -(-threads // 64)
    per_simd = -(-waves // SIMDS)
    regs = -(-max(r["vgpr"], r["agpr"]) // GRANULE) * GRANULE
    return per_simd, per_simd * regs


def fit(members):
    """members: [(record, threads, dynamic LDS bytes)] -> (fits one CU together, explanation)"""
    waves = regs = lds = 0
    for r, threads, dyn in members:
        w, g = per_simd_regs(r, threads)
        waves += w; regs += g; lds += r["lds"] + dyn
    ok = regs <= REGS_PER_SIMD and lds <= LDS_PER_CU and waves <= WAVES_PER_SIMD
    return ok, "registers %d / %d per SIMD lane, LDS %d / %d bytes, waves %d / %d per SIMD" % (regs, REGS_PER_SIMD, lds, LDS_PER_CU, waves, WAVES_PER_SIMD)


def test_launch_shapes_the_budget_assumes_are_the_library_s():
    """The block sizes and dynamic LDS used here are the ones the hybrid launches with: a change there must update this test."""
    xf = open(os.path.join(CSRC, "te_xfwd.hip")).read()
    te = open(os.path.join(CSRC, "tile_engine.hip")).read()
    assert re.search(r"#define XS %d\b" % XS, xf)
    assert "(size_t)2 * XS * 16 * (D + 16) + (size_t)NW * 3 * KB * SL * 64 * 16" in xf
    assert "KB = D / 64, NW = D / 16, SL = XS - 3" in xf
    assert "static dim3 block() { return dim3(F64 ? D * 2 : D * 4); }" in xf
    hyb_f = xf[xf.index("(the split: te_hybrid_kernel)"):]
    hyb_f = hyb_f[:hyb_f.index("done = true;")]
    for ft in ("true", "false"):
        assert "te_rec_fwd1x_kernel<D, false, %s>), dim3(min(n, num_cu)), dim3(4 * D), 0, A.side2, A)" % ft in hyb_f
        assert "XRec<D>::template launch<%s, false>(A, st)" % ft in hyb_f
    hyb_b = te[te.index("(the split: te_scan)"):]
    hyb_b = hyb_b[:hyb_b.index("} else")]
    assert "te_rec_bwd1_kernel<D>, dim3(min(n, num_cu)), dim3(4 * D), 0, s2, A)" in hyb_b
    assert "(te_rec_bwd16t_kernel<D>), dim3((n + 15) / 16), dim3(D * 4), sizeof(short) * (3 * 16 * (3 * D + 16) + 3 * D * D), st, A)" in hyb_b
    ab = open(os.path.join(CSRC, "abi.hip")).read()
    assert re.search(r"A\.hyb = \(.*D == 128 &&", ab), "the hybrid is no longer dim 128 only: extend pairs() to the new dims"


def test_every_instance_is_in_the_library(kernels):
    for name in NAMES:
        assert name in kernels, "kernel %s not found in the library (renamed? update pairs())" % name
        r = kernels[name]
        assert r["vgpr"] >= r["agpr"], (name, r)          # unified count (see the module docstring)


def test_each_kernel_fits_a_cu_alone(kernels):
    for D in (64, 128):
        for (a, da), (b, db) in pairs(D):
            for name, dyn in ((a, da), (b, db)):
                ok, why = fit([(kernels[name], 4 * D, dyn)])
                assert ok, "%s cannot even run: %s" % (name, why)


def test_hybrid_pairs_at_dim_128_never_share_a_cu(kernels):
    for (a, da), (b, db) in pairs(128):
        ok, why = fit([(kernels[a], 4 * 128, da), (kernels[b], 4 * 128, db)])
        print("%s + %s: %s" % (a, b, why))
        assert not ok, "one workgroup of %s and one of %s fit ONE CU together (%s): the hybrid recurrences are no longer bitwise reproducible" % (a, b, why)


def test_capacity_model_sees_the_dim_64_co_residency(kernels):
    """The control: at dim 64 (256-thread workgroups, one wave per SIMD) the backward pair DOES fit one CU - the co-residency behind the
    nondeterminism that keeps the hybrid off at dim 64.  A model that never finds a fit would pass the dim-128 test for nothing."""
    (a, da), (b, db) = pairs(64)[2]
    ok, why = fit([(kernels[a], 4 * 64, da), (kernels[b], 4 * 64, db)])
    print("%s + %s: %s" % (a, b, why))
    assert ok, why
