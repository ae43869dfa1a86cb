"""The launch planner of the fused top-K scoring (csrc/score_plan.h) compiled on its own, against the rules it replaced - the path
choice that abi_serve.hip::score_common, score_filter.hip's launchers and the support / size functions next to the kernels used to work
out between them - re-spelled here in Python from that code, on a grid that crosses every boundary of the rules."""
import itertools
import random
import shutil
import subprocess

import pytest

import poi_amd
from tests.score_plan_cases import CASES, K

NONE, PROB, BINS8, BINS16, GEO = range(5)
PRE = {0: "none", 1: "prefix", 2: "maxpass"}
FIELDS = ("variant d8 n_split lds_one_stage gbound seeded two_stage pre sub_tiles pre_split bins ut nsf lds_filter lds_rescore nsm max_stride items "
          "items_chunk items_grid lds_items b_items_pk b_cand_s b_cand_i b_gbound b_pre_idx b_pre_sc b_items_pk16 b_inorm b_surv_cnt b_surv_idx b_surv_sc "
          "b_tflag b_users_pk16 b_ubound b_ugeo").split()

_MAIN = r"""
#include <stdio.h>
#include "score_plan.h"
int main() {
  int n, n_item, dim, k, dist, n_dist, all, seed_k, num_cu, variant, filter, sf_items, nsplit;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &n, &n_item, &dim, &k, &dist, &n_dist, &all, &seed_k, &num_cu, &variant, &filter, &sf_items, &nsplit) == 13) {
    const ScoreShape S = {n, n_item, dim, k, dist, n_dist, all != 0, seed_k};
    const ScoreSettings C = {num_cu, variant, filter, sf_items, nsplit};
    const ScorePlan P = plan_score(S, C);
    printf("%d %d %d %zu %d %d %d %d %d %d %d %d %d %zu %zu %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", P.variant, P.d8, P.n_split,
           P.lds_one_stage, (int)P.gbound, (int)P.seeded, (int)P.two_stage, P.pre, P.sub_tiles, P.pre_split, P.bins, P.ut, P.nsf, P.lds_filter, P.lds_rescore, P.nsm,
           P.max_stride, (int)P.items, P.items_chunk, P.items_grid, P.lds_items, P.b_items_pk, P.b_cand_s, P.b_cand_i, P.b_gbound, P.b_pre_idx, P.b_pre_sc, P.b_items_pk16,
           P.b_inorm, P.b_surv_cnt, P.b_surv_idx, P.b_surv_sc, P.b_tflag, P.b_users_pk16, P.b_ubound, P.b_ugeo);
  }
  return 0;
}
"""

WAVETOPK = 32 * 80 * 4 + 32 * 80 * 2 + 4 * 32 * 4      # struct WaveTopk of score_topk.hip: cs, ci, cnt / thr / gseen / gtmp
SF_CAP = 4096


def _before(n, n_item, dim, k, dist, n_dist, all_scores, seed_k, num_cu, score_variant, topk_filter, sf_items, nsplit):
    """What the code before the planner did with this call, in its order: score_common, then the launchers.  A field the old code never
    reached is 0."""
    geo, resident, prob = dist == GEO, dist in (BINS8, BINS16), dist == PROB
    ntile, n_utile = (n_item + 31) // 32, (n + 31) // 32
    n_pad = n_utile * 32
    r = dict.fromkeys(FIELDS, 0)

    def geo_stream_lds():
        d8 = 16 if dim <= 128 else 32
        return WAVETOPK * 8 + 16 * d8 * 64 + 8 * (n_dist + 96) + 4 * 32

    variant = 1 if (n >= 128 and dim <= 128) else 0
    if score_variant >= 0 and dim <= 128:
        variant = score_variant
    if resident:
        variant = 1
    if geo:
        variant = 0
    if geo and k > 0 and n >= 1024 and dim >= 128 and geo_stream_lds() <= 160 * 1024 and score_variant != 0:
        variant = 2

    def splits_for(nt):
        want = (num_cu * 8 + n_utile - 1) // n_utile
        want = min(want, nt // 8)
        want = max(want, 1)
        want = max(want, (nt + 2046) // 2047)
        return (want + 7) // 8 * 8 if variant == 2 else (want + 3) // 4 * 4

    n_split = splits_for(ntile)
    # the launchers of score_topk.hip: the kernel's k-groups and dynamic LDS
    if variant == 2:
        d8, lds1 = (16 if dim <= 128 else 32), geo_stream_lds()
    else:
        d8 = 4 if dim <= 32 else 8 if dim <= 64 else 16 if dim <= 128 else 32
        lds1 = WAVETOPK * 4 + 16 * d8 * 64 if variant == 1 else (8 * (n_dist + 96) if geo else 0)
    r.update(variant=variant, d8=d8, n_split=n_split, lds_one_stage=lds1)
    if variant:
        r["b_items_pk"] = 4 * 4 * ntile * d8 * 64
    if k <= 0:
        return r
    cand = n_split * n_pad * k
    seeded = seed_k >= k and seed_k <= 64
    supported = k > 0 and not prob and not all_scores and n >= 128 and n_dist + 1 <= 1024 and (dim in (64, 128, 256) if geo else dim in (64, 128))
    two_stage = bool(topk_filter) and (variant == 1 or geo) and supported
    sub_tiles = 0 if not two_stage else ((ntile // 16 if ntile >= 256 else 0) if not seeded else (ntile // 64 if n_item >= (1 << 20) else 0))
    if two_stage and not seeded and sub_tiles == 0:
        two_stage = False
    gbound = n_split > 1 or seeded or two_stage
    if gbound:
        r["b_gbound"] = 4 * n_pad
    maxpass = two_stage and not seeded and sub_tiles > 0 and (not geo and dim in (64, 128) and 0 < k <= 64 and ntile >= 64 * 4)
    pre = 0
    if two_stage and sub_tiles > 0 and not maxpass:
        pre = 1
        r["b_pre_idx"] = r["b_pre_sc"] = 4 * n_pad * k
        r["sub_tiles"], r["pre_split"] = sub_tiles, splits_for(sub_tiles)
        cand = max(cand, r["pre_split"] * n_pad * k)                    # the regrow in the middle of the call
    elif maxpass:
        pre = 2
    r.update(gbound=int(gbound), seeded=int(seeded), two_stage=int(two_stage), pre=pre, b_cand_s=4 * cand, b_cand_i=4 * cand)
    if not two_stage:
        return r
    kg = dim // 16
    r.update(b_items_pk16=16 * ntile * kg * 64, b_inorm=8 * ntile * 32, b_surv_cnt=4 * n_pad, b_surv_idx=4 * n_pad * SF_CAP, b_surv_sc=4 * n_pad * SF_CAP, b_tflag=4 * n_utile)
    items = 1 if (geo and n_item >= (1 << 20) and n_utile <= 4096) else 0
    if sf_items >= 0:                                                   # poi_ctx_set_topk_filter(2 / 3), or POI_SF_ITEMS behind it
        items = sf_items if geo else 0
    nsf = (4 * num_cu + n_utile - 1) // n_utile * 4
    nsf = max(nsf, 16)
    if nsplit >= 4:
        nsf = nsplit // 4 * 4
    nsf = min(nsf, ntile // 4 * 4)
    nsf = max(nsf, 4)
    # launch_two_stage_t / launch_maxpass_t
    bins = 3 if geo else 1 if dist == BINS8 else 2 if dist == BINS16 else 0
    per_tile = 4 * (kg * 64 * 4 + 128 + (((32 * (n_dist + 1) + 3) & ~3) if bins else 0))
    ut = 2 if (not geo and 2 * per_tile <= 79 * 1024) else 1
    r.update(bins=bins, ut=ut, nsf=nsf, lds_filter=ut * per_tile + (8 * (n_dist + 96) + 4 * 32 if geo else 0), lds_rescore=4 * (dim // 8) * 64 * 4, items=items)
    if items:
        chunk = (1 << 20) // (kg * 1024)
        units = ((ntile + 3) // 4) * ((n_utile + chunk - 1) // chunk)
        r.update(items_chunk=chunk, items_grid=min(units, num_cu * 2), lds_items=16 * 2 * kg * 64 + 4 * (64 + 4) + 8 * (2 * 96 + n_dist + 2) + 4 * (n_utile + 4),
                 b_users_pk16=16 * n_utile * kg * 64, b_ubound=16 * n_pad, b_ugeo=24 * n_pad)
    if maxpass:
        r.update(nsm=64 if nsf >= 64 else 32 if nsf >= 32 else 16, max_stride=2 if ntile >= 64 * 8 else 1)
    return r


def _refused(n, n_item, dim, k, dist, n_dist, all_scores, seed_k, *settings):
    """Combinations no entry point lets through to the planner."""
    if k > n_item or (k == 0) != bool(all_scores):
        return True
    if dist in (NONE, PROB):
        return n_dist != 0
    if k == 0 or n_dist <= 0:                           # the bin paths are top-K calls
        return True
    if dist in (BINS8, BINS16) and (dim > 128 or n * (n_dist + 1) >= 1 << 31):
        return True
    return dist == BINS8 and n_dist > 255


N_USERS = (1, 127, 128, 1023, 1024, 4096, 4096 * 32, 4096 * 32 + 1, 65536)      # (4096: the only way to 32 ranges of the block-maximum pass)
N_ITEMS = tuple(32 * t - 7 for t in (1, 3, 4, 255, 256, 257)) + ((1 << 20) - 1, 1 << 20, 10 ** 7)
DIMS = (4, 32, 36, 64, 68, 128, 132, 256)
KS = (0, 1, 20, 32)
N_DISTS = (0, 200, 255, 256, 400, 401, 1023, 1024)
SETTINGS = list(itertools.product((1, 256, 304), (-1, 0, 1), (1, 0), (-1, 0, 1), (0, 3, 4, 10, 4096)))      # num_cu, score_variant, topk_filter, items override, nsf override
DEFAULTS = (256, -1, 1, -1, 0)


def _shapes(seeds):
    out = [(n, ni, d, k, dist, nd, int(k == 0), s) for n, ni, d, k, dist, nd in itertools.product(N_USERS, N_ITEMS, DIMS, KS, range(5), N_DISTS) for s in seeds(k)]
    return [s for s in out if not _refused(*s)]


def _grid():
    """Every shape, unseeded and seeded, under the default settings; every setting and every kind of seed on the shapes at the rules'
    boundaries; and a fixed random sample of the full product of shapes, seeds and settings."""
    plain = _shapes(lambda k: (0, k) if k else (0,))
    every = _shapes(lambda k: sorted({0, max(k - 1, 0), k, 64, 65}))
    cases = [s + DEFAULTS for s in plain]
    edge = lambda s: s[0] in (128, 1024, 4096 * 32 + 1) and s[1] in (32 * 256 - 7, 32 * 257 - 7, 1 << 20) and s[2] in (128, 256) and s[3] == 20 and s[5] in (0, 200, 400, 401)
    cases += [s + c for s in plain if edge(s) for c in SETTINGS]
    cases += [s + (cu, -1, f, -1, 0) for s in every if edge(s) for cu in (1, 256, 304) for f in (1, 0)]
    rnd = random.Random(20)
    cases += [s + rnd.choice(SETTINGS) for s in rnd.sample(every, len(every) // 16)]
    return cases


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_plan")
    cxx = shutil.which("c++") or shutil.which("g++") or poi_amd.build._hipcc()
    src, exe = str(d / "score_plan_main.cpp"), str(d / "score_plan_main")
    open(src, "w").write(_MAIN)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", poi_amd.build.CSRC, src, "-o", exe], check=True)      # alone: no HIP anywhere near it

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        got = [dict(zip(FIELDS, (int(v) for v in line.split()))) for line in out if line]
        assert len(got) == len(cases)
        return got
    return run


@pytest.fixture(scope="module")
def planned(planner):
    """(cases, the planner's plans), computed once."""
    cases = _grid()
    return cases, planner(cases)


def test_plan_score_reproduces_the_rules_it_replaced(planned):
    cases, got = planned
    want = [_before(*c) for c in cases]
    for c, g, w in zip(cases, got, want):
        assert g == w, (c, {f: (g[f], w[f]) for f in FIELDS if g[f] != w[f]})
    # every regime and every boundary is in the grid
    assert {w["variant"] for w in want} == {0, 1, 2} and {w["pre"] for w in want} == {0, 1, 2} and {w["ut"] for w in want} == {0, 1, 2}
    assert {(w["seeded"], w["pre"]) for w in want} >= {(1, 1), (0, 1), (0, 2), (1, 0)}              # (1, 1): the seeded prefix regime of a table of 2^20 items
    assert {w["items"] for w in want if w["two_stage"]} == {0, 1} and {w["nsm"] for w in want} == {0, 16, 32, 64} and {w["max_stride"] for w in want} == {0, 1, 2}
    # (the range count grows with the tiles, so the prefix pass never needed more candidate lists than the main pass: the regrow the old code
    # carried for that case did not trigger anywhere on this grid; the planner still sizes the lists for the larger of the two)
    assert all(w["pre_split"] <= w["n_split"] for w in want)
    geo256 = {c[5]: w["variant"] for c, w in zip(cases, want) if c[4] == GEO and c[2] == 256 and c[0] == 1024 and c[8:] == DEFAULTS}
    assert geo256[400] == 2 and geo256[401] == 0                                                      # score_geo_stream_lds crosses 160 KB


def test_plan_score_keeps_what_the_kernels_rely_on(planned):
    for c, p in zip(*planned):
        n, n_item, k = c[0], c[1], c[3]
        ntile = (n_item + 31) // 32
        # 16-bit item offsets in the candidate lists: fewer than 65536 items per range, main pass and prefix pass
        assert -(-ntile // p["n_split"]) * 32 < 65536, (c, p)
        assert p["n_split"] % (8 if p["variant"] == 2 else 4) == 0 and p["n_split"] >= 4, (c, p)
        if p["pre"] == 1:
            assert 0 < p["sub_tiles"] <= ntile and -(-p["sub_tiles"] // p["pre_split"]) * 32 < 65536, (c, p)
            assert p["pre_split"] % (8 if p["variant"] == 2 else 4) == 0, (c, p)
            assert p["b_cand_s"] == 4 * max(p["n_split"], p["pre_split"]) * ((n + 31) // 32 * 32) * k, (c, p)
        else:
            assert p["sub_tiles"] == 0 and p["pre_split"] == 0, (c, p)
        if p["variant"] == 2:
            assert p["lds_one_stage"] <= 160 * 1024, (c, p)
        if p["two_stage"]:
            assert p["nsf"] % 4 == 0 and p["nsf"] >= 4 and (p["seeded"] or p["pre"]), (c, p)
            assert max(p["lds_one_stage"], p["lds_filter"], p["lds_rescore"]) <= 160 * 1024, (c, p)
            assert p["lds_items"] <= 64 * 1024, (c, p)                       # (score_filter_items_kernel never raises its limit)
            assert p["ut"] == (1 if p["bins"] == 3 else p["ut"]) and (p["bins"], p["ut"]) != (0, 1), (c, p)      # the (BINS, UT) kernels that exist
            if p["pre"] == 2:
                assert p["nsm"] in (16, 32, 64) and p["nsm"] * 32 <= SF_CAP and p["bins"] != 3, (c, p)      # block maxima live in a user's survivor-score slots
            if p["items"]:
                assert p["bins"] == 3 and 1 <= p["items_grid"] <= 2 * c[8] and p["items_chunk"] >= 1, (c, p)
        else:
            assert p["pre"] == 0 and p["nsf"] == 0 and p["b_surv_idx"] == 0, (c, p)


def test_the_case_table_names_the_planners_regimes(planner):
    """tests/score_plan_cases.py, which the GPU test holds the launch counts against: on the 256 CUs of an MI355X."""
    dist = {"plain": NONE, "all": NONE, "bins8": BINS8, "geo": GEO}
    seed_k = {None: 0, "true": K, "short": 10}
    rows = [(c["n"], c["n_item"], c["dim"], 0 if c["call"] == "all" else K, dist[c["call"]], c["n_dist"], int(c["call"] == "all"), seed_k[c["seed"]],
             256, -1, int(c["filt"] is not False), 1 if c["filt"] == "items" else -1, 0) for c in CASES]
    for c, p in zip(CASES, planner(rows)):
        got = dict(variant=p["variant"], two_stage=bool(p["two_stage"]), pre=PRE[p["pre"]], seeded=bool(p["seeded"]), items=bool(p["items"]))
        assert got == c["regime"], (c["name"], got, c["regime"])
