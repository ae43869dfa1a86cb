"""The case table of the fused top-K scoring's launch plan (csrc/score_plan.h), shared by tests/test_score_plan_cpu.py (the planner gives
every case the regime named here) and tests/test_gpu_score_plan.py (the call launches what the regime implies, and returns the one-stage
lists).  K = 20 throughout; the regimes assume the 256 CUs of an MI355X only where stated.

call    plain = poi_score_topk, bins8 = poi_score_topk_ulptai with uint8 bins, geo = poi_score_topk_geo, all = poi_score_all
seed    None, "true" (the true lists, seed_k = K) or "short" (their first 10 columns: seed_k < K does not count)
filt    what Context.set_topk_filter takes: True, False or "items" (item-stationary GEO filter forced)
regime  variant (one-stage kernel), two_stage, pre (the self-seeding pre-pass: none / prefix / maxpass), seeded, items
counts  launches per timing region; regions that are not listed stay at zero"""

K = 20
REGIONS = ("topk_seed", "pack_items", "score_maxpass", "score_filter", "score_rescore", "score_topk", "score_all")


def _case(name, call, n, n_item, dim, n_dist=0, seed=None, filt=True, regime=None, counts=None):
    full = dict.fromkeys(REGIONS, 0)
    full.update(counts)
    return dict(name=name, call=call, n=n, n_item=n_item, dim=dim, n_dist=n_dist, seed=seed, filt=filt, regime=regime, counts=full)


def _regime(variant, two_stage=False, pre="none", seeded=False, items=False):
    return dict(variant=variant, two_stage=two_stage, pre=pre, seeded=seeded, items=items)


_MAXPASS = dict(pack_items=3, score_maxpass=1, score_filter=1, score_rescore=1, score_topk=1)      # f16 block maxima, filter, the one-stage kernel: a pack each
_PREFIX0 = dict(pack_items=1, score_filter=1, score_rescore=1, score_topk=2)                       # the row-per-lane kernel packs nothing

CASES = [
    _case("A", "plain", 96, 3000, 64, regime=_regime(0), counts=dict(score_topk=1)),
    # 94 item tiles: too few for a self-seeding pre-pass, so an unseeded call stays one-stage
    _case("B", "plain", 160, 3000, 64, regime=_regime(1), counts=dict(pack_items=1, score_topk=1)),
    _case("C", "plain", 160, 3000, 64, seed="true", regime=_regime(1, True, seeded=True),
          counts=dict(topk_seed=1, pack_items=2, score_filter=1, score_rescore=1, score_topk=1)),
    _case("D", "plain", 160, 8224, 128, regime=_regime(1, True, "maxpass"), counts=_MAXPASS),      # 257 item tiles
    _case("E", "bins8", 160, 8224, 64, n_dist=200, regime=_regime(1, True, "maxpass"), counts=_MAXPASS),
    _case("F", "geo", 160, 8224, 128, n_dist=200, regime=_regime(0, True, "prefix"), counts=_PREFIX0),
    _case("G", "geo", 160, 8224, 128, n_dist=200, filt="items", regime=_regime(0, True, "prefix", items=True), counts=_PREFIX0),
    # the packed-stream GEO kernel packs for the prefix pass and for the main pass
    _case("H", "geo", 1024, 8224, 128, n_dist=200, regime=_regime(2, True, "prefix"),
          counts=dict(pack_items=3, score_filter=1, score_rescore=1, score_topk=2)),
    _case("I", "plain", 160, 3000, 64, seed="true", filt=False, regime=_regime(1, seeded=True), counts=dict(topk_seed=1, pack_items=1, score_topk=1)),
    _case("J", "plain", 160, 3000, 64, seed="short", regime=_regime(1), counts=dict(pack_items=1, score_topk=1)),
    _case("K", "all", 160, 3000, 64, regime=_regime(1), counts=dict(pack_items=1, score_all=1)),
]
SHORT_SEED_K = 10
