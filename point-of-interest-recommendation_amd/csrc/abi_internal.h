// Shared by the C-ABI translation units (abi.hip, abi_train.hip, abi_serve.hip): the context, its device buffers, the workspace
// carver and the argument checks more than one entry point makes.  Host code only.
#pragma once
#include "../../include/poi_hip.h"
#include "poi_kernels.h"
#include "split_plan.h"
#include "filter_plan.h"
#include "audience_plan.h"
#include "similar_plan.h"

#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)      // nothing here is part of the library's interface

// Device buffer owned by the context: freed with it.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

struct poi_ctx {
  int device = 0;
  int num_cu = 0;
  int wg_per_cu = 2;
  std::string err;
  // per-sequence engine
  DevBuf ws, slab, te_ws, hslab, zrow;
  DevBuf ex_ws, ex_slab, ex_glt, ex_gdi;      // exact (float64) engine
  int engine = 0;   // 0 auto, 1 per-sequence, 2 tile, 3 tile with streaming recurrent kernels, 4 exact (float64)
  float batch_cap = 1.0f;   // poi_ctx_set_batch_cap
  int wgrad_rounds = 2;     // workgroups per CU for te_wgrad (POI_WGRAD_ROUNDS, tuning)
  int head_rounds = 3;      // workgroups per CU for te_head (POI_HEAD_ROUNDS, tuning)
  int score_variant = -1;   // -1 auto; POI_SCORE_VARIANT=0|1 (tuning only)
  DevBuf g_lt, mult_lt, nseq_lt, g_di, mult_di, nseq_di;
  DevBuf g_wd, mult_wd, nseq_wd, ca_ws, ca_slab, ca_scr, ca2;      // CA-RNN (ca2: workspace of the outer-product path)
  int carnn_fast = 1;       // POI_CARNN_FAST=0: the per-sequence kernel with float atomics on the interval matrices (A/B)
  hipEvent_t ev_hr0 = nullptr, ev_hr1 = nullptr;      // early chunk sums of the write-back's hot rows (TeArgs.hot_early)
  int hot_early = 1;        // POI_TE_HOT_EARLY=0: in the tail, as up to round 5 (A/B)
  hipStream_t side2 = nullptr; hipEvent_t ev_h0 = nullptr, ev_h1 = nullptr, ev_h2 = nullptr, ev_h3 = nullptr;      // hybrid recurrences of mid-size launches (TeArgs.hyb)
  int hybrid = 1, hyb_min = 1150, hyb_max = 2300, hyb_force = 0;      // POI_TE_HYBRID=0 / option "hybrid"; launches of hyb_min .. hyb_max sequences (POI_TE_HYB_MIN / _MAX; measured: below ~1200 the per-sequence kernels alone are faster, above ~2600 the tiles alone - the fork / join costs ~15 us)
  hipStream_t side = nullptr; hipEvent_t ev_slots = nullptr, ev_sorted = nullptr, ev_bwd = nullptr, ev_fin = nullptr, ev_start = nullptr, ev_pack = nullptr;   // slot sort next to the GEMMs (POI_TE_SIDE=0: inline)
  DevBuf seg_s, seg_e;      // per table row [start, end) of the sorted scatter (te_scatter.hip); seg_e is all-zero between launches
  DevBuf xc;                // exact forward over the step-input POIs only: rank tables + per-step table rows (TeArgs.xcomp)
  DevBuf pmark;             // per-POI regrouping: per lt row, S row + 1 of a step-input POI of this launch (te_passign; all-zero between launches)
  int ppoi = 1;             // POI_TE_PPOI=0 disables the regrouping (A/B)
  int hot_bins = 1;         // te_psum also sums the DA rows of the most frequent distance bins (TeArgs.dhot); POI_TE_HOTBINS=0 / option "hot_bins"
  int early_bins = 1;       // distance-bin chain of the write-back starts next to te_gemm_dx on the side stream; POI_TE_EARLY_BINS=0: at the tail (A/B)
  int early_min = 1024;     // ... for launches of at least this many sequences (POI_TE_EARLY_MIN; 1300 .. 2000 users: -5 % per launch against the inline chain)
  DevBuf kc_dev;            // te_wgrad's K-chunk split, chosen on the device per launch
  DevBuf ptab, iota;        // forward table (te_rec_fwd16<FT>): lt . ui[:, :D]^T per table row; 0..n_item, n_item + 1
  int iota_n = -1;          // rows the iota buffer currently describes
  int fwd_tab = 1;          // POI_TE_FWDTAB=0 disables (A/B)
  int bintab_min = 1280;    // launches below this many sequences take the two-table path (no per-bin tables / per-POI regrouping); POI_TE_BINTAB_MIN
  int one_path = 1;         // launches of ONE sequence (Distance2Pre, plain GRU) take the five-kernel path (te_one_*); POI_TE_ONE=0 -> the batched pipeline
  int rec1_max = 1800;      // launches of at most this many sequences run the per-sequence recurrent kernels (te_rec_fwd1 / bwd1: persistent since round 5 - crossover with the 16-sequence tiles measured at ~1800 for the backward, ~1100 for the float64 forward pass); POI_TE_REC1
  int rec_split = 1;        // recurrent kernels on bf16 x 3 split operands; POI_TE_SPLIT=0 -> float32-input MFMA (A/B)
  int xlaunch = 0;          // launch id of the exact forward's non-finite-input flag (TeArgs.xflag)
  int xfwd = 1;             // exact forward (te_xfwd.hip: fixed point on the int8 matrix cores / float64 MFMA + float64 gates) for dims 64 / 128 / 256; POI_TE_XFWD=0 / poi_ctx_set_exact_forward
  int xcomp = 1;            // exact forward table over the step-input POIs only; POI_TE_XCOMP=0: every row of the POI table (A/B)
  int xcomp_min = 1536;     // ... for launches of at least this many sequences (below: one row per step - the table form of te_rec_fwdx costs 0.6 us more per step of the latency chain than the ranking saves in te_gemmx; 1300 / 1563 / 2048 / 3125 users: +9 / -6 / -38 / -45 us); POI_TE_XCOMP_MIN
  int xids_lds = 1;         // option "xfwd_ids_lds": the table-form recurrences of the exact forward stage their table-row ids in LDS (TeArgs.xid_cap) instead of loading them inside the step loop; POI_TE_XIDS_LDS=0 (A/B)
  int stream_hints = 1;     // option "stream_hints": the forward recurrence's tiles store the write-once rows G, H, RH non-temporally (TeArgs.stream_hints); POI_TE_STREAM=0 / POI_TE_DBG bit 16384 (A/B)
  int stream_min = 2560;    // ... in launches of at least this many sequences at dim 128, twice as many at dim 64 (option "stream_hints_min"; dim 128, 12500 / 4096 / 2560 users: -38 / -10 / -5 us per launch, 2304 / 1563: +8 / +3 - the rows of a small launch stay on-die for te_rec_bwd; dim 64, 12500 / 4096 / 2560: -36 / +4 / +9)
  int efuse = 1;            // E = lt[p'] - lt[q'] gathered inside te_head3 (dim 128) instead of written by te_gather and read back twice; POI_TE_EFUSE
  int head3 = 1;            // training head on split products for <= 256 bins (te_head3); POI_TE_HEAD3
  int xrec1_max = 1100;     // ... launches of at most this many sequences run its recurrence per sequence in float64 on the vector ALUs (te_rec_fwd1x); POI_TE_XREC1
  DevBuf bad_ids;           // out-of-range ids seen by poi_bpr_step (poi_ctx_take_bad_ids)
  DevBuf xflag;             // launch id of the last launch whose operands held a NaN / inf (TeArgs.xflag)
  DevBuf xw, xg;            // its digit fragments, scales and per-bin table | per-step pre-activations or the forward table (float64)
  // hipGraph replay of the tile engine's training launch (poi_ctx_set_graph): ~40 kernels on two streams become one graph launch.
  // A launch is captured the second time its key (every pointer / size / scalar the kernels receive) is seen; the caller's uidx /
  // out are staged through context buffers so that the key does not depend on them.
  struct StepGraph { std::vector<uint64_t> key; hipGraph_t graph; hipGraphExec_t exec; uint64_t stamp; int fork; };      // fork: the plan record of a replay
  std::vector<StepGraph> graphs;
  std::vector<uint64_t> seen_key;
  int graph_mode = 0;       // off by default (no gain measured on ROCm 7.0: DESIGN.md section 5); POI_GRAPH=1 / poi_ctx_set_graph enable
  int graph_min_n = 0, graph_max_n = 1 << 30;
  uint64_t graph_stamp = 0, graph_replays = 0, graph_captures = 0;
  hipStream_t cap = nullptr;   // capture stream (the caller's stream may be the null stream, which cannot capture)
  DevBuf uidx_stage, out_stage;
  // the plan of the last training launch (poi_ctx_last_plan): host fields, stored where the launch decides them
  struct LastPlan { int valid, tile, one, rec1, xrec1, hyb, bintab, ppoi, listed, fwd_tab, xft, xcomp, xfwd_ids_lds, stream_hints, head_split, efuse, early_bins, fork, cell_kernel, cell_grid, session_path, session_tiles, session_tile_min, near_path, near_splits, near_split_max, rank_splits, geoie_score_span, geoie_score_splits, group_path, group_splits, group_split_max, route_path, route_splits, diverse_path, diverse_splits, diverse_split_max, select_rows_per_chunk, select_chunks, select_path, select_splits, filter_path, filter_splits, filter_split_max, audience_path, audience_splits, audience_split_max, similar_path, similar_splits, similar_split_max, capped_splits, capped_split_max, lists_path, labels_splits, labels_split_max, labels_home, labels_chunks, labels_rows_per_chunk, explain_columns, explain_tiles, explain_start; const int* hyb_dev; hipStream_t st; uint64_t ws_gen; };
  LastPlan plan = {};
  uint64_t te_ws_gen = 0;   // te_setup calls so far: a later one may reuse the workspace that holds plan.hyb_dev
  // BPR
  DevBuf g_ux, g_blt;
  // FPMC-LR step: sort buffers, per-transition sigmoid, window partial sums, new-row slots
  DevBuf fp_ws;
  // PRME step: the same layout for 7 touches per transition
  DevBuf pr_ws;
  // GeoIE step / pair distances: plan, per-row and per-user values, touch gradients, sort buffers, new-row slots
  DevBuf ge_ws;
  // POI2Vec step / scoring scratch
  DevBuf pv_ws, pv_sc;
  DevBuf pv_fold;           // poi_foldin_p2v: float64 running rows, mean target rows, per (user, span) softmax partials
  // mini-batch Lstm / Rnn: packed weights, per-position-row state, sort buffers, chunk partials, new-row slots
  DevBuf cell_ws;
  int cell_grid = 0;        // option "cell_grid": cap of the recurrent kernel's persistent grid (0: none)
  // VBPR step: dense-gradient chunk partials, sort buffers, per-triple values, window partial sums, new-row slots
  DevBuf vb_ws;
  int vbpr_grid = 0;        // option "vbpr_grid": cap of the workgroups of every VBPR kernel (0: none)
  // online sessions: per-slot claims of the repeated-slot check
  DevBuf sess_owner;
  DevBuf sess_wrs;          // poi_session_carnn_advance, tile path: float64 row sums of the interval matrices, rewritten on every call
  int sess_tile_min = 512;  // option "session_tile_min": poi_session_advance calls of at least this many events take the tile kernel
  // restricted top-K (near.hip): per (row, slice) partial lists of the split path
  DevBuf near_ws;
  int near_split_max = 256; // option "near_split_max": poi_score_topk_near calls of at most this many rows split each row's band over several workgroups
  int near_grid = 0;        // option "near_grid": workgroups per row on the split path (0: by the row count and the CUs)
  // GeoIE scoring under the trained rule (geoie_score.hip): per (row, span) partial lists of the top-K mode
  DevBuf geo_ws;
  int geo_span = 0;         // option "geoie_score_span": candidates per workgroup (0: by the row count and the CUs)
  // exact target ranks (rank.hip): the targets' scores and ids, pass 1 -> pass 2
  DevBuf rank_ws;
  int rank_grid = 0;        // option "rank_grid": cap of the item ranges a 32-row tile is split into (0: by the row count and the CUs)
  // group recommendation (group.hip): per (group, slice) partial lists of the split path
  DevBuf group_ws;
  int group_split_max = 256; // option "group_split_max": poi_group_topk calls of at most this many groups cut the item range into slices, a workgroup each
  int group_grid = 0;       // option "group_grid": slices on the split path (0: by the group count and the CUs)
  // route recommendation (route.hip): per (row, wave range) partial lists, per (row, item block) normaliser partials, row status
  DevBuf route_ws;
  int route_split_max = 8192; // option "route_split_max": poi_route_expand calls of at most this many rows cut the item range of every 32-row tile over several workgroups
  int route_grid = 0;       // option "route_grid": workgroups per 32-row tile on the split path (0: by the row count and the CUs)
  // diversified recommendation (diverse.hip): per (row, slice) partial lists of the split path; poi_diverse_topk's pool between its two stages
  DevBuf diverse_ws;
  int diverse_split_max = 256; // option "diverse_split_max": poi_diverse_pool calls of at most this many rows cut the item range of every 32-row tile into slices, a workgroup each
  int diverse_grid = 0;     // option "diverse_grid": slices on the split path (0: by the row count and the CUs)
  // candidate generation (select.hip): the score rows of a chunk (poi_score_candidates); per-row histograms, state and candidate slots
  DevBuf select_sc, select_ws;
  int select_split_max = 256; // option "select_split_max": calls of at most this many rows cut each row's id range into slices, a workgroup each
  int select_grid = 0;      // option "select_grid": slices on the split path (0: by the row count and the CUs)
  int select_chunk_mb = 1024; // option "select_chunk_mb": poi_score_candidates keeps at most this many MiB of score rows at a time
  // filtered recommendation (filter.hip): per (row, slice) partial lists of the split regime
  DevBuf filter_ws;
  int filter_split_max = 256; // option "filter_split_max": poi_score_topk_filtered calls of at most this many rows cut the item range (walk) / every row's candidates (gather) into slices, a workgroup each
  int filter_grid = 0;      // option "filter_grid": slices in the split regime (0: by the row count and the CUs)
  int filter_gather_cost = FILTER_GATHER_COST_DEFAULT;      // option "filter_gather_cost": POI_FILTER_AUTO's price of a gathered candidate in walk cells (filter_plan.h)
  // audience recommendation (audience.hip): per (query, slice) partial lists of the split regime
  DevBuf audience_ws;
  int audience_split_max = 256; // option "audience_split_max": poi_score_audience / poi_audience_rows calls of at most this many queries cut the candidate rows into slices, a workgroup each per query block
  int audience_grid = 0;    // option "audience_grid": slices in the split regime (0: by the query-block count and the CUs)
  // similar rows (similar.hip): per (query, slice) partial lists of the split regime; the row norms of a call without inv_norm; the score rows of the rows + select route
  DevBuf similar_ws, similar_inv, similar_sc;
  int similar_split_max = SIMILAR_SPLIT_MAX_DEFAULT; // option "similar_split_max": poi_similar_topk / poi_similar_rows calls of at most this many queries cut the table's rows into slices, a workgroup each per query block
  int similar_grid = 0;     // option "similar_grid": slices in the split regime (0: by the query-block count and the CUs)
  int similar_rows_max = SIMILAR_ROWS_MAX_DEFAULT;      // option "similar_rows_max": poi_similar_topk calls of at most this many queries go through score rows + selection
  // capped recommendation (capped.hip): poi_labels_build's label histograms; per (row, slice) partial lists of the split regime
  DevBuf capped_ws;
  int capped_split_max = 256; // option "capped_split_max": poi_score_topk_capped calls of at most this many rows cut the item range of every 32-row tile into slices, a workgroup each
  int capped_grid = 0;      // option "capped_grid": slices in the split regime (0: by the row count and the CUs)
  int capped_hist_kb = 256 << 10; // option "capped_hist_kb": poi_labels_build keeps at most this many KiB of label histograms at a time (whole predicates, at least one)
  // label recommendation (labels.hip): the accumulators of a chunk of rows - per (row, bucket) mass, best key and count, per row M and status
  DevBuf labels_ws;
  int labels_split_max = 256; // option "labels_split_max": calls of at most this many rows cut the item range of every 32-row tile into slices, a workgroup each
  int labels_grid = 0;      // option "labels_grid": slices in the split regime (0: by the row count and the CUs)
  int labels_lds_kb = 40;   // option "labels_lds_kb": the accumulators of a workgroup live in LDS while 32 (n_label + 1) 20 bytes fit this many KiB (0: always in global memory); not measured yet
  int labels_ws_kb = 256 << 10; // option "labels_ws_kb": the accumulator workspace holds at most this many KiB (whole 32-row tiles, at least one); more rows go through it in chunks
  // leave-one-out attribution (explain.hip): the rows' bad-id flags and the base states after every 16th position
  DevBuf explain_ws;
  int explain_start = 1;    // option "explain_start": 1 - a variant starts from the base walk's checkpoint before its first removed position; 0 - at position 0 from h = 0
  // re-ranking (rerank.hip): the rejected-row flags of poi_score_lists; poi_rerank's scores between its two stages
  DevBuf rerank_ws;
  // scoring
  DevBuf cand_s, cand_i, items_pk, gbound;
  DevBuf items_pk16, inorm, surv_cnt, surv_idx, surv_sc, tflag, pre_idx, pre_sc;      // two-stage fused top-K (score_filter.hip)
  DevBuf users_pk16, ubound, ugeo;      // item-stationary GEO filter: users' half fragments, per-user bound terms, last-POI coordinates
  int sf_items = -1;        // poi_ctx_set_topk_filter(ctx, 2 / 3): force / forbid the item-stationary GEO filter (-1: POI_SF_ITEMS, then by shape)
  int sf_items_env = -1;    // POI_SF_ITEMS=1|0: the same, for A/B runs (-1: by shape)
  int sf_nsplit = 0;        // POI_SF_NSPLIT=<n>: item ranges of the filter pass (tuning; below 4: by shape)
  int score_dbg = 0;        // POI_SCORE_DBG: ScoreArgs.dbg (tuning, 0 in production)
  int f16_rounding = 0;     // poi_ctx_set_f16_rounding: 0 nearest, 1 stochastic (write-back of a half POI table)
  unsigned sr_counter = 0;  // launches so far (salt of the stochastic rounding)
  int topk_filter = 1;      // poi_ctx_set_topk_filter / POI_TOPK_FILTER=0: one-stage float32 kernel only
  int last_two_n = 0, last_two_tiles = 0;      // users / user tiles of the last two-stage call (poi_ctx_topk_filter_stats)
  const int32_t* seed_idx = nullptr; int seed_k = 0;      // poi_ctx_set_topk_seed: consumed by the next fused top-K call
  // selftest
  DevBuf st;
  poi::Timing tm;
  std::vector<std::pair<const char*, size_t>> f16;      // registered IEEE-half table buffers (poi_ctx_register_f16)
};

// defined in abi.hip
int is_f16(const poi_ctx* c, const void* p);
int fail(poi_ctx* c, int code, const char* fmt, ...);
int ensure(poi_ctx* c, DevBuf& b, size_t bytes, hipStream_t st);
void drop_graphs(poi_ctx* c);
double shortest_decimal(float x);
double lat_band_deg(double c);

#define HIPCHK(c, expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(c, POI_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

// Pieces of one device buffer, each rounded up to 256 bytes.  On a null base it only counts.
struct Carver {
  char* base; size_t used = 0;
  explicit Carver(void* p) : base((char*)p) {}
  void* bytes(size_t b) { void* r = base ? (void*)(base + used) : nullptr; used += (b + 255) & ~(size_t)255; return r; }
};

// One description of a workspace: `layout` runs on a counting Carver, the buffer grows to what it took, `layout` runs again on the buffer.
template <class Layout>
int carve(poi_ctx* c, DevBuf& b, hipStream_t st, Layout&& layout) {
  Carver dry(nullptr);
  layout(dry);
  int rc = ensure(c, b, dry.used + 256, st);
  if (rc) return rc;
  Carver W(b.p);
  layout(W);
  return POI_OK;
}

// The pieces every sort-based step has (launch_radix_sort and the chunk / span kernels): four key / value arrays of per * n touches
// (+ 64 spare) each, the radix histogram with the element counters right behind it, one int4 per 64-touch window.
template <class Args>
void carve_sort(Args& A, Carver& W, int per, size_t n, size_t chunks) {
  const size_t T = (size_t)per * n + 64;
  A.keys0 = (int*)W.bytes(sizeof(int) * 4 * T); A.keys1 = A.keys0 + T; A.vals0 = A.keys0 + 2 * T; A.vals1 = A.keys0 + 3 * T;
  A.hist = (int*)W.bytes(sizeof(int) * ((size_t)RS_HIST_INTS + RS_MAXBIN + 64)); A.cnt = A.hist + RS_HIST_INTS + RS_MAXBIN;
  A.meta = (int4*)W.bytes(sizeof(int4) * chunks);
}

// Partial top-K lists of a split path: per list k_max scores, k_max ids and one count.
template <class Args>
int carve_lists(poi_ctx* c, DevBuf& b, hipStream_t st, Args& A, size_t lists, int k_max) {
  return carve(c, b, st, [&](Carver& W) {
    A.part_s = (float*)W.bytes(sizeof(float) * lists * k_max);
    A.part_i = (int*)W.bytes(sizeof(int) * lists * k_max);
    A.part_cnt = (int*)W.bytes(sizeof(int) * lists);
  });
}

// The operand block tile_operands() (abi_serve.hip) has filled, into a family's argument struct: the same members under the same names.
template <class Args>
void put_operands(Args& A, const poi::TileOperands& T) {
  A.users = T.users; A.items = T.items; A.items_f16 = T.items_f16; A.n = T.n; A.n_item = T.n_item; A.dim = T.dim;
  A.wd = T.wd; A.sts = T.sts; A.coords = T.coords; A.cphi = T.cphi; A.thr = T.thr; A.last_poi = T.last_poi; A.n_dist = T.n_dist; A.bin_scale = T.bin_scale;
  A.ex_off = T.ex_off; A.ex = T.ex; A.bad = T.bad;
}

// Argument checks shared by the entry points (defined in abi.hip).  Each returns POI_OK or the code it has recorded with fail().
int refuse_batch_cap0(poi_ctx* c);      // the mini-batch rule is the GRU steps' alone
int bad_counter(poi_ctx* c, hipStream_t st, int** bad);      // the context's counter of out-of-range ids (poi_ctx_take_bad_ids)
int check_ex_pair(poi_ctx* c, const char* who, const void* ex_off, const void* ex, const char* verb = "go");
// the optional distance term: ptrs_ok - the arrays that come with wd are there (else "who: ptr_msg"); n_dist > 0 and dd > 0; *bin_scale
// is the kernels' metres-per-bin factor, 0 without the term
int check_geo_term(poi_ctx* c, const char* who, bool geo, bool ptrs_ok, const char* ptr_msg, int n_dist, double dd, float* bin_scale);
// per-model parameter checks used by both a step and a scoring entry (defined in abi_train.hip)
int prme_check(poi_ctx* c, const poi_prme_params* P, const char* who);
int geoie_check(poi_ctx* c, const poi_geoie_params* P, const char* who);
int poi2vec_check(poi_ctx* c, const poi_poi2vec_params* P, const char* who);

#pragma GCC visibility pop
