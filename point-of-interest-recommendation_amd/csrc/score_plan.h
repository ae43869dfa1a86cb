// The launch plan of the fused scoring / top-K calls (poi_score_all, poi_score_topk, poi_score_topk_ulptai, poi_score_topk_geo): which
// kernels run, with what grids, LDS sizes and buffers - decided once per call from its shape and the context's settings, before anything
// is allocated or launched (abi_serve.hip::score_common).  Plain host arithmetic, no HIP: a test compiles it on its own.
#pragma once
#include <stddef.h>

// what the kernels and this arithmetic share (score_topk.hip, score_filter.hip)
#define TK_CAP 80   // candidate slots per user per wave (>= K + 32; compaction when cnt > TK_CAP - 32).
                    // 4 waves x 32 users x 80 x 6 B = 61 KB per workgroup (+ 16 KB of A fragments: two workgroups per CU)
#define SG_NW 8     // waves per workgroup of score_kernel_geo_stream
#define SF_CAP 4096       // survivor slots per user in global memory (good seeds leave ~K + 1 of them, the self-seeding pre-pass ~16 K; an overflow flags the tile).  8 bytes per slot: a 65536-user call pins 2 GB of grow-only context memory
#define SCORE_WAVETOPK_BYTES (32 * TK_CAP * 6 + 4 * 32 * 4)      // sizeof(WaveTopk) (score_topk.hip asserts it)
#define SCORE_LDS_MAX (160 * 1024)

enum { SCORE_DIST_NONE = 0, SCORE_DIST_PROB = 1, SCORE_DIST_BINS8 = 2, SCORE_DIST_BINS16 = 3, SCORE_DIST_GEO = 4 };      // the distance term
enum { SCORE_PRE_NONE = 0, SCORE_PRE_PREFIX = 1, SCORE_PRE_MAXPASS = 2 };      // self-seeding pre-pass of the two-stage path

struct ScoreShape {
  int n, n_item, dim, k;      // k = 0: all scores, no lists
  int dist, n_dist;           // SCORE_DIST_*; n_dist = 0 without bins
  bool all_scores;            // the (n, n_item) score matrix is wanted
  int seed_k;                 // ids per user of the caller's seed (poi_ctx_set_topk_seed), 0 = none
};
struct ScoreSettings {
  int num_cu;
  int score_variant;          // -1 auto, 0 / 1 forced (POI_SCORE_VARIANT)
  int topk_filter;            // two-stage path allowed
  int sf_items;               // item-stationary GEO filter: -1 by shape, 0 forbidden, 1 forced
  int sf_nsplit;              // item ranges of the filter pass (POI_SF_NSPLIT), below 4 = by shape
};
struct ScorePlan {
  int variant, d8, n_split;   // one-stage kernel: 0 row-per-lane, 1 packed stream, 2 packed-stream GEO; k-groups of 8; item ranges per user tile
  size_t lds_one_stage;
  bool gbound, seeded;        // shared per-user bounds in use; the caller's seed counts
  bool two_stage;
  int pre, sub_tiles, pre_split;      // SCORE_PRE_*; item tiles and item ranges of the prefix pass
  int bins, ut, nsf;          // filter: BINS of score_filter_kernel, user tiles per workgroup, item ranges
  size_t lds_filter, lds_rescore;
  int nsm, max_stride;        // block-maximum pass: item ranges (16 / 32 / 64), every max_stride-th item tile
  bool items;                 // item-stationary filter
  int items_chunk, items_grid; size_t lds_items;
  // bytes of the context's buffers (0: not used by this call)
  size_t b_items_pk, b_cand_s, b_cand_i, b_gbound, b_pre_idx, b_pre_sc;
  size_t b_items_pk16, b_inorm, b_surv_cnt, b_surv_idx, b_surv_sc, b_tflag, b_users_pk16, b_ubound, b_ugeo;
};

// k-groups of 8 of the item fragments a variant's kernel walks (the packed table has d8 x 64 float4 per item tile)
inline int score_d8(int variant, int dim) { return variant == 2 ? (dim <= 128 ? 16 : 32) : dim <= 32 ? 4 : dim <= 64 ? 8 : dim <= 128 ? 16 : 32; }

// score_kernel_geo_stream: eight waves' candidate lists, the user tile's A fragments, thresholds + user coordinates, largest distance terms
inline size_t score_geo_stream_lds(int dim, int n_dist) {
  return (size_t)SCORE_WAVETOPK_BYTES * SG_NW + 16 * (size_t)score_d8(2, dim) * 64 + sizeof(double) * (size_t)(n_dist + 96) + sizeof(float) * 32;
}
// dynamic LDS of the one-stage kernel of a variant (variant 0 keeps its candidate lists in static LDS)
inline size_t score_one_stage_lds(int variant, int dim, bool geo, int n_dist) {
  if (variant == 2) return score_geo_stream_lds(dim, n_dist);
  if (variant == 1) return (size_t)SCORE_WAVETOPK_BYTES * 4 + 16 * (size_t)score_d8(1, dim) * 64;
  return geo ? sizeof(double) * (size_t)(n_dist + 96) : 0;
}

// item ranges per user tile for a table of nt item tiles: long item streams keep per-user thresholds high (few top-K compactions)
inline int score_splits(int num_cu, int n_utile, int nt, int variant) {
  int want = (num_cu * 8 + n_utile - 1) / n_utile;   // 8 waves per CU
  if (want > nt / 8) want = nt / 8;          // >= 8 tiles per stream: amortise the per-wave top-K epilogue
  if (want < 1) want = 1;
  if (want < (nt + 2046) / 2047) want = (nt + 2046) / 2047;      // candidate lists hold 16-bit item offsets: < 65536 items per range
  return variant == 2 ? ((want + 7) / 8) * 8 : ((want + 3) / 4) * 4;
}

// what the two-stage path (score_filter.hip) can run at all; a prob matrix and the score matrix are the one-stage kernels' alone
inline bool score_two_stage_supported(const ScoreShape& S) {
  if (!(S.k > 0 && S.dist != SCORE_DIST_PROB && !S.all_scores && S.n >= 128 && S.n_dist + 1 <= 1024)) return false;
  return S.dist == SCORE_DIST_GEO ? (S.dim == 64 || S.dim == 128 || S.dim == 256) : (S.dim == 64 || S.dim == 128);      // (the users' bin probabilities live in LDS: 32 x (n_dist + 1) floats)
}
inline bool score_maxpass_supported(const ScoreShape& S) {
  return S.dist != SCORE_DIST_GEO && (S.dim == 64 || S.dim == 128) && S.k > 0 && S.k <= 64 && (S.n_item + 31) / 32 >= 64 * 4;
}

// score_filter_kernel, per user tile: [dim / 16][64] half fragments | 4 x 32 per-user terms | 32 x (n_dist + 1) bin probabilities (bins)
inline size_t score_filter_tile_lds(int dim, int n_dist, bool bins) {
  return sizeof(float) * ((size_t)(dim / 16) * 64 * 4 + 128 + (bins ? ((32 * (size_t)(n_dist + 1) + 3) & ~(size_t)3) : 0));
}
// user tiles per workgroup: two while both fit twice into a CU's LDS (two workgroups per CU), else one
inline int score_filter_ut(int dim, int n_dist, bool bins, bool geo) { return (!geo && 2 * score_filter_tile_lds(dim, n_dist, bins) <= 79 * 1024) ? 2 : 1; }
inline size_t score_filter_lds(int dim, int n_dist, bool bins, bool geo) {
  return score_filter_ut(dim, n_dist, bins, geo) * score_filter_tile_lds(dim, n_dist, bins) + (geo ? sizeof(double) * (size_t)(n_dist + 96) + sizeof(float) * 32 : 0);
}

// item-stationary filter: user tiles per chunk - ~1 MB of half fragments, which then live in the L2 of every XCD (score_filter_items_kernel)
constexpr int score_items_chunk(int dim) { return (1 << 20) / ((dim / 16) * 1024); }
inline size_t score_items_lds(int dim, int n_dist, int n_utile) {
  return 16 * 2 * (size_t)(dim / 16) * 64 + sizeof(float) * (64 + 4) + sizeof(double) * (2 * 96 + (size_t)n_dist + 2) + sizeof(int) * ((size_t)n_utile + 4);
}

inline ScorePlan plan_score(const ScoreShape& S, const ScoreSettings& C) {
  ScorePlan P = {};
  const int n = S.n, n_item = S.n_item, dim = S.dim, k = S.k;
  const bool geo = S.dist == SCORE_DIST_GEO, resident = S.dist == SCORE_DIST_BINS8 || S.dist == SCORE_DIST_BINS16;
  const int ntile = (n_item + 31) / 32, n_utile = (n + 31) / 32;
  const size_t n_pad = (size_t)n_utile * 32;
  // variant: 0 = one item stream per wave (row-per-lane loads; small n or dim > 128), 1 = packed item
  // stream per wave with the user tile's A fragments in LDS (default for n >= 128)
  P.variant = (n >= 128 && dim <= 128) ? 1 : 0;
  if (C.score_variant >= 0 && dim <= 128) P.variant = C.score_variant;
  if (resident) P.variant = 1;      // the bin matrix is laid out for the packed-stream kernel
  if (geo) P.variant = 0;           // bins on the fly: the row-per-lane kernel (any dim <= 256)
  // ... or, for enough users to fill the chip with eight-wave workgroups and a wide model, the packed-stream GEO kernel
  if (geo && k > 0 && n >= 1024 && dim >= 128 && score_geo_stream_lds(dim, S.n_dist) <= SCORE_LDS_MAX && C.score_variant != 0) P.variant = 2;
  P.d8 = score_d8(P.variant, dim);
  P.n_split = score_splits(C.num_cu, n_utile, ntile, P.variant);
  P.lds_one_stage = score_one_stage_lds(P.variant, dim, geo, S.n_dist);
  if (P.variant) P.b_items_pk = sizeof(float) * 4 * (size_t)ntile * P.d8 * 64;
  if (k <= 0) return P;

  P.seeded = S.seed_k >= k && S.seed_k <= 64;      // (seed_k = 0: no seed; k >= 1)
  P.two_stage = C.topk_filter && (P.variant == 1 || geo) && score_two_stage_supported(S);
  // SELF-SEEDING pre-pass of the two-stage path: the one-stage kernel on the first 1/16 of the item tiles (1/64 when the caller's
  // seed already gave bounds) - the K-th best EXACT score of any subset is a lower bound of the final K-th best, so the filter pass
  // starts from thresholds that leave ~16 K (64 K) survivors per user whatever the seed holds: an unseeded call (the first evaluation
  // of a run) or a useless seed (a model that moved a lot) no longer sends its tiles to the one-stage kernel.  Unseeded calls always
  // take it; seeded ones when the table has >= 2^20 items (there it costs < 2 % of the call).
  P.sub_tiles = !P.two_stage ? 0 : !P.seeded ? (ntile >= 256 ? ntile / 16 : 0) : (n_item >= (1 << 20) ? ntile / 64 : 0);
  if (P.two_stage && !P.seeded && P.sub_tiles == 0) P.two_stage = false;      // (a small table and no seed: one-stage)
  P.gbound = P.n_split > 1 || P.seeded || P.two_stage;
  // unseeded, resident bin matrix / no distance term, dims 64 / 128: thresholds from the block maxima of the f16 lower bounds instead
  // (score_filter.hip, MAXP: one f16 pass over ALL items, ~1.3 K survivors per user against ~17 K of the float32 prefix pre-pass)
  if (P.two_stage && P.sub_tiles > 0) P.pre = (!P.seeded && score_maxpass_supported(S)) ? SCORE_PRE_MAXPASS : SCORE_PRE_PREFIX;
  if (P.pre != SCORE_PRE_PREFIX) P.sub_tiles = 0;
  else P.pre_split = score_splits(C.num_cu, n_utile, P.sub_tiles, P.variant);
  // the candidate lists serve the main pass and the prefix pass: sized once, for the larger of the two
  const size_t cand = (size_t)(P.pre_split > P.n_split ? P.pre_split : P.n_split) * n_pad * k;
  P.b_cand_s = sizeof(float) * cand; P.b_cand_i = sizeof(int) * cand;
  if (P.gbound) P.b_gbound = sizeof(unsigned) * n_pad;
  if (P.pre == SCORE_PRE_PREFIX) { P.b_pre_idx = sizeof(int) * n_pad * k; P.b_pre_sc = sizeof(float) * n_pad * k; }
  if (!P.two_stage) return P;

  // two-stage: f16 filter pass + exact float32 rescoring of the survivors (score_filter.hip)
  const size_t kg = dim / 16;
  P.bins = geo ? 3 : S.dist == SCORE_DIST_BINS8 ? 1 : S.dist == SCORE_DIST_BINS16 ? 2 : 0;
  P.ut = score_filter_ut(dim, S.n_dist, P.bins != 0, geo);
  P.lds_filter = score_filter_lds(dim, S.n_dist, P.bins != 0, geo);
  P.lds_rescore = sizeof(float) * ((size_t)(dim / 8) * 64 * 4);
  P.b_items_pk16 = 16 * (size_t)ntile * kg * 64; P.b_inorm = sizeof(float) * 2 * (size_t)ntile * 32;
  P.b_surv_cnt = sizeof(int) * n_pad; P.b_surv_idx = sizeof(int) * n_pad * SF_CAP; P.b_surv_sc = sizeof(float) * n_pad * SF_CAP;
  P.b_tflag = sizeof(int) * (size_t)n_utile;
  // GEO with a huge item table and few users (config X's evaluation): the item-stationary filter - every user tile's own pass over the
  // item table is 1.3 TB at 8192 users x 10 M POIs
  P.items = geo && (C.sf_items >= 0 ? C.sf_items != 0 : (n_item >= (1 << 20) && n_utile <= 4096));
  if (P.items) {
    P.items_chunk = score_items_chunk(dim);
    const long long units = (long long)((ntile + 3) / 4) * ((n_utile + P.items_chunk - 1) / P.items_chunk);      // (four item tiles, chunk of user tiles)
    P.items_grid = units < C.num_cu * 2 ? (int)units : C.num_cu * 2;
    P.lds_items = score_items_lds(dim, S.n_dist, n_utile);
    P.b_users_pk16 = 16 * (size_t)n_utile * kg * 64; P.b_ubound = sizeof(float) * 4 * n_pad; P.b_ugeo = sizeof(double) * 3 * n_pad;
  }
  P.nsf = ((4 * C.num_cu + n_utile - 1) / n_utile) * 4;      // >= 4 workgroups (16 waves) per CU
  if (P.nsf < 16) P.nsf = 16;      // (swept at the Gowalla shape: 8 / 16 / 32 / 64 / 128 ranges -> 3.09 / 2.84 / 2.80 / 2.86 / 3.21 ms of filter time)
  if (C.sf_nsplit >= 4) P.nsf = (C.sf_nsplit / 4) * 4;      // tuning switch
  if (P.nsf > (ntile / 4) * 4) P.nsf = (ntile / 4) * 4;
  if (P.nsf < 4) P.nsf = 4;
  if (P.pre == SCORE_PRE_MAXPASS) {
    P.nsm = P.nsf >= 64 ? 64 : P.nsf >= 32 ? 32 : 16;      // 512 .. 2048 blocks per user
    // every second item tile: the K-th largest block maximum over half of the items is about the 2 K-th best score - 40 survivors per user
    // instead of 21 for half of this pass (measured at the Gowalla shape, strides 1 / 2 / 4 / 8: 6.5 / 5.2 / 5.3 / 6.6 ms per unseeded call)
    P.max_stride = ntile >= 64 * 8 ? 2 : 1;
  }
  return P;
}
