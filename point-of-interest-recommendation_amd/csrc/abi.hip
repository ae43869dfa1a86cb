// C-ABI of libpoi_hip.so (see include/poi_hip.h): context, scratch ownership, argument checks,
// kernel dispatch.  No torch types, no host allocation handed to the caller.
#include "../../include/poi_hip.h"
#include "poi_kernels.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

namespace {
thread_local std::string g_err;
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
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
  int wgrad_rounds = 2;
  int head_rounds = 3;      // workgroups per CU for te_head (POI_HEAD_ROUNDS, tuning)     // workgroups per CU for te_wgrad (POI_WGRAD_ROUNDS, tuning)
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
  struct LastPlan { int valid, tile, one, rec1, xrec1, hyb, bintab, ppoi, listed, fwd_tab, xft, xcomp, head_split, efuse, early_bins, fork, cell_kernel, cell_grid, session_path, session_tiles, session_tile_min, near_path, near_splits, near_split_max, rank_splits, geoie_score_span, geoie_score_splits, group_path, group_splits, group_split_max; const int* hyb_dev; hipStream_t st; uint64_t ws_gen; };
  LastPlan plan = {};
  uint64_t te_ws_gen = 0;   // te_setup calls so far: a later one may reuse the workspace that holds plan.hyb_dev
  // BPR
  DevBuf g_ux, cnt_ux, g_blt, cnt_blt;
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
  // scoring
  DevBuf cand_s, cand_i, items_pk, gbound;
  DevBuf items_pk16, inorm, surv_cnt, surv_idx, surv_sc, tflag, pre_idx, pre_sc;      // two-stage fused top-K (score_filter.hip)
  DevBuf users_pk16, ubound, ugeo;      // item-stationary GEO filter: users' half fragments, per-user bound terms, last-POI coordinates
  int sf_items = -1;        // poi_ctx_set_topk_filter(ctx, 2 / 3): force / forbid the item-stationary GEO filter (-1: by shape)
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

static int is_f16(const poi_ctx* c, const void* p) {
  if (!c || !p) return 0;
  for (auto& r : c->f16) if ((const char*)p >= r.first && (const char*)p < r.first + r.second) return 1;
  return 0;
}

static int fail(poi_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(c, POI_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

// Grow-only zero-initialised device buffer.  Contents are all-zero after (re)allocation; users
// of gradient tables rely on that and restore the zeros themselves after each launch.
static int ensure(poi_ctx* c, DevBuf& b, size_t bytes, hipStream_t st) {
  if (bytes <= b.bytes) return POI_OK;
  if (b.p) { HIPCHK(c, hipStreamSynchronize(st)); HIPCHK(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
  size_t want = bytes + bytes / 8;
  if (hipMalloc(&b.p, want) != hipSuccess) {
    (void)hipGetLastError();
    want = bytes;
    if (hipMalloc(&b.p, want) != hipSuccess) { b.p = nullptr; return fail(c, POI_ENOMEM, "hipMalloc(%zu) failed", bytes); }
  }
  b.bytes = want;
  HIPCHK(c, hipMemsetAsync(b.p, 0, want, st));
  return POI_OK;
}

extern "C" {

int poi_abi_version(void) { return POI_ABI_VERSION; }

const char* poi_last_error(const poi_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int poi_ctx_create(poi_ctx** out, int device) {
  if (!out) return fail(nullptr, POI_EINVAL, "poi_ctx_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, POI_EHIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(nullptr, POI_EINVAL, "device %d out of range (%d visible)", device, ndev);
  poi_ctx* c = new poi_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete c; return fail(nullptr, POI_EHIP, "hipGetDeviceProperties failed"); }
  c->num_cu = prop.multiProcessorCount;
  if (const char* e = getenv("POI_SEQ_WG_PER_CU")) { int v = atoi(e); if (v >= 1 && v <= 8) c->wg_per_cu = v; }
  if (const char* e = getenv("POI_HEAD_ROUNDS")) { int v = atoi(e); if (v >= 1 && v <= 4) c->head_rounds = v; }
  if (const char* e = getenv("POI_WGRAD_ROUNDS")) { int v = atoi(e); if (v >= 1 && v <= 4) c->wgrad_rounds = v; }
  if (const char* e = getenv("POI_SCORE_VARIANT")) { int v = atoi(e); if (v >= 0 && v <= 1) c->score_variant = v; }
  if (const char* e = getenv("POI_TE_PPOI")) c->ppoi = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_EARLY_BINS")) c->early_bins = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_HOTBINS")) c->hot_bins = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_HYBRID")) c->hybrid = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_HOT_EARLY")) c->hot_early = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_HYB_MIN")) c->hyb_min = atoi(e);
  if (const char* e = getenv("POI_TE_HYB_MAX")) c->hyb_max = atoi(e);
  if (const char* e = getenv("POI_TE_HYB_FORCE")) c->hyb_force = atoi(e);
  if (const char* e = getenv("POI_TE_EARLY_MIN")) c->early_min = atoi(e);
  if (const char* e = getenv("POI_TE_FWDTAB")) c->fwd_tab = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_SPLIT")) c->rec_split = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_XFWD")) c->xfwd = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_XREC1")) c->xrec1_max = atoi(e);
  if (const char* e = getenv("POI_TE_HEAD3")) c->head3 = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_EFUSE")) c->efuse = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_XCOMP")) c->xcomp = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_XCOMP_MIN")) c->xcomp_min = atoi(e);
  if (const char* e = getenv("POI_TE_REC1")) c->rec1_max = atoi(e);
  if (const char* e = getenv("POI_TE_ONE")) c->one_path = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_BINTAB_MIN")) c->bintab_min = atoi(e);
  if (const char* e = getenv("POI_CARNN_FAST")) c->carnn_fast = atoi(e) != 0;
  if (const char* e = getenv("POI_GRAPH")) c->graph_mode = atoi(e) != 0;
  if (const char* e = getenv("POI_TOPK_FILTER")) c->topk_filter = atoi(e) != 0;
  if (const char* e = getenv("POI_ENGINE")) { if (!strcmp(e, "seq")) c->engine = 1; else if (!strcmp(e, "tile")) c->engine = 2; else if (!strcmp(e, "exact")) c->engine = 4; }
  if (hipSetDevice(device) != hipSuccess) { delete c; return fail(nullptr, POI_EHIP, "hipSetDevice failed"); }
  const char* sd = getenv("POI_TE_SIDE");
  if (!sd || atoi(sd) != 0) {
    // (a high or a low stream priority for the side stream changes nothing: 1727 - 1746 us per 12500-user launch either way)
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_slots, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_sorted, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_bwd, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fin, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_hr0, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_hr1, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      c->side = nullptr;                     // fall back to the inline sort
    }
    if (c->side && (hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_h0, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&c->ev_h1, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&c->ev_h2, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_h3, hipEventDisableTiming) != hipSuccess)) {
      (void)hipGetLastError();
      c->side2 = nullptr;                    // no hybrid recurrences
    }
  }
  if (c->graph_mode && hipStreamCreateWithFlags(&c->cap, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->cap = nullptr; c->graph_mode = 0; }
  *out = c;
  return POI_OK;
}

static void drop_graphs(poi_ctx* c) {
  for (auto& g : c->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
  c->graphs.clear(); c->seen_key.clear();
}

int poi_ctx_destroy(poi_ctx* c) {
  if (!c) return POI_OK;
  DevBuf* all[] = {&c->ex_ws, &c->ex_slab, &c->ex_glt, &c->ex_gdi, &c->ws, &c->slab, &c->te_ws, &c->hslab, &c->zrow, &c->g_lt, &c->mult_lt, &c->nseq_lt, &c->g_di, &c->mult_di, &c->nseq_di, &c->seg_s, &c->seg_e, &c->pmark, &c->xc, &c->kc_dev, &c->uidx_stage, &c->out_stage, &c->ptab, &c->iota, &c->xw, &c->xg, &c->xflag, &c->bad_ids,
                   &c->g_wd, &c->mult_wd, &c->nseq_wd, &c->ca_ws, &c->ca_slab, &c->ca_scr, &c->ca2, &c->g_ux, &c->cnt_ux, &c->g_blt, &c->cnt_blt, &c->cand_s, &c->cand_i, &c->items_pk, &c->gbound, &c->st,
                   &c->items_pk16, &c->inorm, &c->surv_cnt, &c->surv_idx, &c->surv_sc, &c->tflag, &c->pre_idx, &c->pre_sc, &c->users_pk16, &c->ubound, &c->ugeo, &c->fp_ws, &c->pr_ws, &c->ge_ws, &c->pv_ws, &c->pv_sc, &c->pv_fold, &c->cell_ws, &c->vb_ws, &c->rank_ws, &c->sess_wrs, &c->geo_ws, &c->group_ws};
  (void)hipDeviceSynchronize();
  c->tm.clear();
  drop_graphs(c);
  if (c->cap) (void)hipStreamDestroy(c->cap);
  if (c->side2) { (void)hipStreamDestroy(c->side2); (void)hipEventDestroy(c->ev_h0); (void)hipEventDestroy(c->ev_h1); (void)hipEventDestroy(c->ev_h2); (void)hipEventDestroy(c->ev_h3); }
  if (c->side) { (void)hipStreamDestroy(c->side); (void)hipEventDestroy(c->ev_slots); (void)hipEventDestroy(c->ev_sorted); (void)hipEventDestroy(c->ev_bwd); (void)hipEventDestroy(c->ev_fin); (void)hipEventDestroy(c->ev_start); (void)hipEventDestroy(c->ev_pack); (void)hipEventDestroy(c->ev_hr0); (void)hipEventDestroy(c->ev_hr1); }
  for (DevBuf* b : all) if (b->p) (void)hipFree(b->p);
  delete c;
  return POI_OK;
}

int poi_ctx_num_cu(const poi_ctx* c) { return c ? c->num_cu : POI_EINVAL; }

// ---------------------------------------------------------------------------------------------
static int check_gru(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, bool spatial, bool need_q) {
  if (!c || !P || !T) return fail(c, POI_EINVAL, "NULL ctx/params/tables");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "dim must be a multiple of 4 in [4, 256] (got %d)", P->dim);
  if (!P->lt || !P->ui || !P->wh || !P->bi) return fail(c, POI_EINVAL, "lt/ui/wh/bi must be non-NULL");
  if (spatial && (!P->di || !P->vs || !P->bs || !P->wd || !P->lw || P->n_dist <= 0)) return fail(c, POI_EINVAL, "spatial model needs di/vs/bs/wd/lw and n_dist > 0");
  if (!T->off || !T->p) return fail(c, POI_EINVAL, "tables: off/p must be non-NULL");
  if (need_q && !T->q) return fail(c, POI_EINVAL, "tables: q must be non-NULL");
  if (spatial && (!T->dp || (need_q && !T->dq))) return fail(c, POI_EINVAL, "tables: dp/dq must be non-NULL for the spatial model");
  if (T->max_len <= 0 || T->len_max < T->max_len) return fail(c, POI_EINVAL, "tables: need 0 < max_len <= len_max");
  return POI_OK;
}

static void fill_args(poi::SeqArgs& A, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int n) {
  memset(&A, 0, sizeof A);
  A.lt = P->lt; A.di = P->di; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.vs = P->vs; A.bs = P->bs; A.wd = P->wd; A.lw = P->lw;
  A.n_item = P->n_item; A.n_dist = P->n_dist; A.dim = P->dim;
  A.off = T->off; A.p = T->p; A.q = T->q; A.dp = T->dp; A.dq = T->dq;
  A.len_max = T->len_max; A.cap = T->max_len;
  A.uidx = uidx; A.n_seq = n;
  A.bcap = 1.0f;
}

// Carve the tile engine's packed-row workspace out of one grow-only buffer.
static int te_setup(poi_ctx* c, poi::TeArgs& A, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int n,
                    bool predict, bool spatial, hipStream_t st) {
  memset(&A, 0, sizeof A);
  ++c->te_ws_gen;
  const int n_dist = spatial ? P->n_dist : -1;            // the plain GRU has no distance-bin table: zero rows
  const int D = P->dim, NBP = poi::te_nbp(n_dist);
  A.lt = P->lt; A.di = P->di; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.vs = P->vs; A.bs = P->bs; A.wd = P->wd; A.lw = P->lw;
  A.n_item = P->n_item; A.n_dist = n_dist; A.dim = D;
  A.spatial = spatial ? 1 : 0; A.xw = spatial ? 2 * D : D;
  A.lt_f16 = is_f16(c, P->lt);
  A.bintab = (poi::te_bintab(D, spatial, n_dist) && (predict || n >= c->bintab_min)) ? 1 : 0;
  A.rec32 = (D >= 256 || (D == 128 && c->engine == 3)) ? 1 : 0;
  A.rec_split = c->rec_split ? 1 : 0;          // (16-sequence tiles and the streaming kernels of dim 256 alike)
  A.head_split = (c->rec_split && A.spatial && (P->n_dist + 1 > 256 || (c->head3 && !predict))) ? 1 : 0;      // (<= 256 bins: te_head3, training launches only)
  A.efuse = (c->efuse && A.head_split && !predict && P->n_dist + 1 <= 256 && D == 128) ? 1 : 0;      // (the one-sequence path clears it: te_one_in writes E)
  A.rec1 = (!A.rec32 && n <= c->rec1_max) ? 1 : 0;
  // hybrid recurrences (poi_kernels.h TeArgs.hyb): training launches of hyb_min .. hyb_max sequences on the exact forward, dim 128.  (NOT dim 64: there a
  // workgroup of each kernel fits the same CU, and with the two backward kernels co-resident identical launches differed in the last bits of DA in 5 - 20 % of
  // the runs - inside every parity bar, but not bitwise reproducible; serialised, or at dim 128 where each workgroup fills its CU, 0 of 240: tools/repro_check.py)
  A.hyb = (c->hybrid && c->side2 && !predict && !A.rec32 && D == 128 && c->xfwd && poi::te_xfwd_supported(D) && c->rec_split && n >= c->hyb_min && n <= c->hyb_max && n <= TE_HYB_NMAX && n > 1) ? 1 : 0;
  A.hyb_force = c->hyb_force;
  if (A.hyb) A.rec1 = 0;                    // (the tile kernels' weight packs; the per-sequence backward kernel gets its transposes in pWhc1 / pWhzr1)
  A.ppoi = (A.bintab && !predict && c->ppoi) ? 1 : 0;
  A.off = T->off; A.p = T->p; A.q = T->q; A.dp = T->dp; A.dq = T->dq; A.len_max = T->len_max;
  A.uidx = uidx; A.n_seq = n; A.predict = predict ? 1 : 0;
  if (const char* e = getenv("POI_TE_DBG")) A.dbg = atoi(e);
  A.dl = poi::dense_layout(D, A.xw, n_dist + 1);
  const size_t Tcap = (size_t)n * (size_t)(predict ? T->max_len : (T->max_len > 1 ? T->max_len - 1 : 1)) + 192;   // + spare rows: row T and the rest of the last 128-row tile
  // uiT 6 + uiP 3 + pWhT16 4.5 + pWhc16 1.5 + pWhzr16 3 + pUiP3 4.5 (x D^2) + spare, pVsT + pVs 2 x 1.5 NBP D, + the rounding of each carve
  const size_t pk = (size_t)30 * D * D + (size_t)3 * NBP * D + 128;      // (+ 3 D^2: pWhc1 / pWhzr1 of the hybrid recurrences)
  // sorted scatter (training): 3 slots per sequence position
  const bool sorted = !predict;
  const size_t Ncap = sorted ? 3 * (Tcap + (size_t)n) : 0;
  const size_t n_hot = Ncap / (TE_COLD_MAX + 1) + 2, n_chunk = Ncap / TE_HOT_CHUNK + n_hot + 2;
  const size_t sfl = sorted ? Tcap + n_chunk * D + Tcap * (size_t)NBP + (size_t)((n <= c->rec1_max || n <= c->hyb_max) ? n : (n + 15) / 16) * 3 * D + (size_t)2 * ((n + 255) / 256) + 128 : 0;
  const int Rrows = P->n_item + 1 + n_dist + 1;
  const bool listed = sorted && (size_t)Rrows > 4 * Ncap;      // table much larger than the launch's footprint: touched-row list
  const size_t sin = sorted ? 7 * Ncap + (listed ? Ncap : 0) + (size_t)RS_HIST_INTS + RS_MAXBIN + 16 + 4 * n_hot + 3 * n_chunk + 64 : 0;
  // per-bin tables (bintab): ztab + per-bin sums + d di sums, and (training) the sliced partial sums of DA
  const size_t NBt = (size_t)(n_dist + 1), n_dchunk = (Tcap + (size_t)n) / 64 + NBt + 2 + (size_t)TE_HB * (size_t)TE_PSUM_WG;      // (+ the hot bins' per-workgroup partials: TeArgs.dhot)
  A.npw = TE_PSUM_WG;         // workgroups of te_psum: a CONSTANT (the hot bins' partial sums are formed per workgroup: their summation order must not depend on the device's CU count); 96 registers x 384 threads - three or four of them fit a CU at a time      // 64-entry chunks of the bins' entry segments
  const size_t n_dsuper = n_dchunk / 32 + NBt + 2;
  const size_t bfl = A.bintab ? NBt * (size_t)(3 * D) * 2 + NBt * D + (sorted ? (n_dchunk + n_dsuper) * (size_t)(3 * D) : 0) + 64 : 0;
  const size_t n_prange = Tcap / 64 + 4;
  const size_t pfl = A.ppoi ? Tcap * (size_t)(3 * D) + 2 * n_prange * (size_t)(3 * D) + 64 : 0;
  const size_t nfl = Tcap * (size_t)(9 * D + 2) + pk + 64 + sfl + bfl + pfl;
  const size_t nin = Tcap * 7 + (size_t)n + 48 + sin + 512 + (A.bintab && sorted ? n_dchunk + n_dsuper + 4 * NBt + 64 : 0) + 3 * NBt + 48 + (A.ppoi ? 4 * Tcap + 2 * 1024 + 128 : 0);
  int rc = ensure(c, c->te_ws, nfl * 4 + nin * 4 + 1024, st);
  if (rc) return rc;
  const int R = P->n_item + 1 + n_dist + 1;
  if (sorted && ((rc = ensure(c, c->seg_s, sizeof(int) * (size_t)(R + 1), st)) || (rc = ensure(c, c->seg_e, sizeof(int) * (size_t)(R + 1), st)))) return rc;
  if (A.ppoi && (rc = ensure(c, c->pmark, sizeof(int) * (size_t)(P->n_item + 2), st))) return rc;
  // forward table: worth it when the table has clearly fewer rows than the launch has steps (Tcap is the upper bound: sequences
  // average ~40 % of the longest) - te_gemm_ax then multiplies n_item + 1 rows instead of one row per step
  // exact forward (dims 64 / 128): input product and forward recurrence in fixed point / float64 (te_xfwd.hip)
  // dim 256 (config X): the streaming backward kernels keep their 32-sequence tiles, the forward pass runs te_gemmx<256> + te_rec_fwdd (float64 MFMA)
  A.xfwd = (c->xfwd && (!A.rec32 || D == 256) && poi::te_xfwd_supported(D)) ? 1 : 0;      // (training launches and predict alike)
  const bool want_ft = c->fwd_tab && !A.rec32 && 2 * (size_t)(P->n_item + 1) <= Tcap;
  A.fwd_tab = (!A.xfwd && want_ft && A.bintab && !A.rec1) ? 1 : 0;      // (the per-sequence kernels read G)
  A.xrec1 = (A.xfwd && D <= 128 && n <= c->xrec1_max && !A.hyb) ? 1 : 0;      // one workgroup per sequence, float64 on the vector ALUs (te_rec_fwd1x)
  // (the table over the launch's step-input POIs only - te_slots marks them for the per-POI regrouping - never has more rows than the launch has steps)
  const bool want_xc = c->xcomp && A.ppoi && P->n_item + 1 <= (1 << 22) && n >= c->xcomp_min;
  A.xft = (A.xfwd && (want_ft || want_xc) && n > 1) ? 1 : 0;      // (n == 1: the one-sequence path writes gx itself, te_one_in; the per-sequence kernel has a table variant too)
  if (A.fwd_tab || A.xft) {
    if ((rc = ensure(c, c->iota, sizeof(int) * (size_t)(P->n_item + 8), st))) return rc;
    if (c->iota_n != P->n_item + 1) { poi::launch_te_iota((int*)c->iota.p, P->n_item + 1, st); c->iota_n = P->n_item + 1; }
    A.iota = (const int*)c->iota.p;
  }
  if (A.fwd_tab) {
    // (+ spare rows: te_gemm_ntk writes whole 128-row tiles - rows past the table's last land behind it, as in G)
    if ((rc = ensure(c, c->ptab, sizeof(float) * ((size_t)(P->n_item + 1 + 127) / 128 * 128 + 128) * 3 * D, st))) return rc;
    A.ptab = (float*)c->ptab.p;
  }
  if (A.xfwd) {
    const size_t frag = (size_t)3 * D * D * 5, nz = (size_t)(spatial ? n_dist + 1 : 1) * 3 * D;      // five int8 digit planes per weight
    if ((rc = ensure(c, c->xw, 2 * frag + 64 + sizeof(double) * (6 * (size_t)D + nz + 8) + 64, st))) return rc;
    A.xcomp = (A.xft && want_xc) ? 1 : 0;
    const size_t xrows = A.xcomp ? std::min((size_t)P->n_item + 1, Tcap) + 2 : A.xft ? (size_t)P->n_item + 1 + 2 : Tcap;
    if ((rc = ensure(c, c->xg, sizeof(double) * xrows * 3 * D, st))) return rc;
    char* xp = (char*)c->xw.p;
    A.xWh8 = (uint4*)xp; A.xUi8 = (uint4*)(xp + ((frag + 15) & ~(size_t)15));
    double* xd = (double*)(xp + 2 * ((frag + 15) & ~(size_t)15));
    A.xWhS = xd; A.xUiS = xd + 3 * D; A.ztabx = xd + 6 * D;
    // (its own allocation: the address must not move with the dim / bin count of the launch - whatever an earlier launch left at a recycled
    // offset would be read as a launch id; zero-filled at allocation, ids start at 1)
    if ((rc = ensure(c, c->xflag, 64, st))) return rc;
    A.xflag = (int*)c->xflag.p; A.xlaunch = ++c->xlaunch;
    if (A.xft) A.ptabx = (double*)c->xg.p; else A.gx = (double*)c->xg.p;
    A.x_rows_est = (int)(Tcap < (size_t)1 << 30 ? Tcap : (size_t)1 << 30);
    if (A.xcomp) {
      const size_t nr = ((size_t)P->n_item + 2 + 3) & ~(size_t)3;
      if ((rc = ensure(c, c->xc, sizeof(int) * (2 * nr + 256 + 8 + Tcap), st))) return rc;
      int* xi = (int*)c->xc.p;
      A.xidx = xi; A.xlist = xi + nr; A.xblk = xi + 2 * nr; A.xcnt = xi + 2 * nr + 256; A.row_pc = xi + 2 * nr + 256 + 8;
    }
  }
  float* f = (float*)c->te_ws.p;
  auto take = [&](size_t cnt) { float* r = f; f += (cnt + 3) & ~(size_t)3; return r; };
  A.X = take(Tcap * 2 * D); A.E = take(Tcap * D); A.G = take(Tcap * 3 * D); A.H = take(Tcap * D);
  A.RH = take(Tcap * D); A.DH = take(Tcap * D); A.rowloss = take(Tcap * 2);
  A.uiT = take((size_t)6 * D * D); A.uiP = take((size_t)3 * D * D);
  A.pUiP3 = (float4*)take((size_t)9 * D * D / 2);
  A.pVsT = (float4*)take((size_t)NBP * D * 3 / 2); A.pVs = (float4*)take((size_t)NBP * D * 3 / 2);      // (x 1.5: te_head_big3 reads bf16 x 3 planes)
  // (x 1.5: the split-operand recurrent kernels keep every weight as three bf16 planes)
  A.pWhT16 = (float4*)take((size_t)9 * D * D / 2); A.pWhc16 = (float4*)take((size_t)3 * D * D / 2); A.pWhzr16 = (float4*)take((size_t)3 * D * D);
  if (A.hyb) { A.pWhc1 = (float4*)take((size_t)D * D); A.pWhzr1 = (float4*)take((size_t)2 * D * D); } else { A.pWhc1 = A.pWhc16; A.pWhzr1 = A.pWhzr16; }
  if (A.bintab) {
    A.ztab = take(NBt * 3 * D); A.dsum = take(NBt * 3 * D); A.dgd = take(NBt * D);
    if (sorted) { A.dpart = take(n_dchunk * (size_t)(3 * D)); A.dpart2 = take(n_dsuper * (size_t)(3 * D)); }
  }
  if (A.ppoi) { A.S = take(Tcap * (size_t)(3 * D)); A.pfirst = take(n_prange * (size_t)(3 * D)); A.plast = take(n_prange * (size_t)(3 * D)); }
  if (sorted) {
    A.gcoef = take(Tcap); A.hot_part = take(n_chunk * D); A.DL = take(Tcap * (size_t)NBP);
    A.bi_part = take((size_t)((A.rec1 || A.hyb) ? n : (n + 15) / 16) * 3 * D); A.fin_part = take((size_t)2 * ((n + 255) / 256) + 8);
  }
  int* ip = (int*)f;
  auto itake = [&](size_t cnt) { int* r = ip; ip += (cnt + 3) & ~(size_t)3; return r; };
  A.hyb_dev = itake(8);
  A.soff = itake(n + 1); A.row_src = itake(Tcap); A.row_t = itake(Tcap); A.row_p = itake(Tcap); A.row_dp = itake(Tcap); A.row_ab = itake(Tcap); A.row_pq = (int2*)itake(2 * Tcap);
  if (sorted) {
    int bits = 1; while ((1 << bits) <= R) ++bits;      // keys 0..R (R = sentinel)
    A.key_bits = bits;
    A.keys0 = itake(Ncap); A.keys1 = itake(Ncap); A.vals0 = itake(Ncap); A.vals1 = itake(Ncap);
    A.code = itake(Ncap); A.slot_seq = itake(Ncap); A.ent = itake(Ncap);
    A.hist = itake(RS_HIST_INTS + RS_MAXBIN);   // + per-digit totals
    A.cnt = itake(8);
    A.urow = listed ? itake(Ncap) : nullptr;
    A.hot_rows = (int4*)itake(4 * n_hot); A.hot_chunks = (int2*)itake(2 * n_chunk); A.hot_nf = itake(n_chunk);
    A.seg_start = (int*)c->seg_s.p; A.seg_end = (int*)c->seg_e.p;
    A.dch0 = itake(NBt + 8); A.dhot = itake(NBt + 16); A.dcc0 = itake(NBt + 8);
    if (A.ppoi) {
      A.urow_p = itake(Tcap); A.pblk = itake(2 * 1024); A.dxe = itake(Tcap); A.dxs = itake(Tcap); A.dstart = itake(Tcap + 4);
      A.pmark = (int*)c->pmark.p;
    }
    if (A.bintab) { A.dch1 = itake(NBt + 8); A.dnf = itake(n_dchunk); A.dnf2 = itake(n_dsuper); A.dbn = itake(NBt + 4); }
  }
  return POI_OK;
}

// auto: the tile engine whenever it supports the shape - measured on MI355X (Gowalla shape, D = 128) it is 4.9x faster than the
// per-sequence engine already at ONE sequence per launch (2.6 k vs 0.53 k steps/s: resident recurrent weights + MFMA against
// GEMVs streamed from L2 by one workgroup), 7x at 16 and 64.  The per-sequence engine serves the other dims / bin counts.
static bool use_tile(const poi_ctx* c, const poi_gru_params* P, bool spatial, int n) {
  (void)n;
  if (c->engine == 1 || c->engine == 4 || !poi::te_supported(P->dim, spatial ? P->n_dist : -1)) return false;
  return true;
}

// The caller's float32 alpha / lambda are the nearest floats to short decimals (0.01, 0.001: prog_bpr_gru_spatial.py:66-67); the
// float64 engine takes the SHORTEST decimal that rounds to the given float - 0.01, not 0.00999999977648 - so that its step equals
// the float64 reference's to rounding, not to 2e-8.
static double shortest_decimal(float x) {
  char buf[64];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)x);
    if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
  }
  return (double)x;
}

static void fill_ex(poi::ExArgs& A, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int n) {
  memset(&A, 0, sizeof A);
  A.lt = P->lt; A.di = P->di; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.vs = P->vs; A.bs = P->bs; A.wd = P->wd; A.lw = P->lw;
  A.n_item = P->n_item; A.n_dist = P->n_dist; A.dim = P->dim;
  A.off = T->off; A.p = T->p; A.q = T->q; A.dp = T->dp; A.dq = T->dq;
  A.len_max = T->len_max; A.cap = T->max_len;
  A.uidx = uidx; A.n_seq = n; A.bcap = 1.0f;
}

// engine 4: float64 arithmetic end to end (exact_engine.hip)
static int exact_step(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n,
                      float alpha, float lambda, float* out, hipStream_t st, bool spatial) {
  if (is_f16(c, P->lt)) return fail(c, POI_ENOTSUP, "the exact engine supports float32 tables only");
  const int D = P->dim, XW = spatial ? 2 * D : D, NB = spatial ? P->n_dist + 1 : 0;
  if (NB > 4096) return fail(c, POI_ENOTSUP, "the exact engine supports at most 4095 distance bins");
  int grid = c->num_cu * c->wg_per_cu;
  if (grid > n) grid = n;
  const poi::DenseLayout dl = poi::dense_layout(D, XW, NB);
  const size_t wsd = poi::ex_ws_doubles(D, NB, T->max_len);
  int rc;
  if ((rc = ensure(c, c->ex_ws, sizeof(double) * wsd * grid, st))) return rc;
  if ((rc = ensure(c, c->ex_slab, sizeof(double) * (size_t)dl.total * grid, st))) return rc;
  if ((rc = ensure(c, c->ex_glt, sizeof(double) * (size_t)(P->n_item + 1) * D, st))) return rc;
  if ((rc = ensure(c, c->mult_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if ((rc = ensure(c, c->nseq_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if (spatial) {
    if ((rc = ensure(c, c->ex_gdi, sizeof(double) * (size_t)(P->n_dist + 1) * D, st))) return rc;
    if ((rc = ensure(c, c->mult_di, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
    if ((rc = ensure(c, c->nseq_di, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
  }
  poi::ExArgs A;
  fill_ex(A, P, T, uidx, n);
  A.out = out; A.bcap = c->batch_cap == 0.0f ? -(float)n : c->batch_cap;
  A.ws = (double*)c->ex_ws.p; A.ws_stride = wsd; A.slab = (double*)c->ex_slab.p;
  A.g_lt = (double*)c->ex_glt.p; A.g_di = (double*)c->ex_gdi.p;
  A.mult_lt = (int*)c->mult_lt.p; A.nseq_lt = (int*)c->nseq_lt.p; A.mult_di = (int*)c->mult_di.p; A.nseq_di = (int*)c->nseq_di.p;
  HIPCHK(c, poi::launch_ex_train(A, spatial, grid, shortest_decimal(alpha), shortest_decimal(lambda), st, &c->tm));
  return POI_OK;
}

static int seq_step(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n,
                    float alpha, float lambda, float* out, void* stream, bool spatial) {
  int rc = check_gru(c, P, T, spatial, true);
  if (rc) return rc;
  if (!uidx || !out || n < 0) return fail(c, POI_EINVAL, "uidx/out NULL or n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.tick();
  c->plan = poi_ctx::LastPlan{}; c->plan.valid = 1;      // (the per-sequence / exact engines: every flag 0)
  if (c->engine == 4) return exact_step(c, P, T, uidx, n, alpha, lambda, out, st, spatial);
  const int D = P->dim, XW = spatial ? 2 * D : D, NB = spatial ? P->n_dist + 1 : 0;
  int grid = c->num_cu * c->wg_per_cu;
  if (grid > n) grid = n;
  const poi::DenseLayout dl = poi::dense_layout(D, XW, NB);
  const size_t wsf = poi::seq_ws_floats(D, NB, T->max_len);
  const bool tile = use_tile(c, P, spatial, n);
  if (!tile && is_f16(c, P->lt)) return fail(c, POI_ENOTSUP, "a half POI table needs the tile engine (dim 64 / 128 / 256, <= 2048 bins)");
  int n_head = 0, n_kc = 0, n_kc_ui = 0, n_slab = grid;
  if (tile) {
    n_head = c->num_cu * (D >= 256 && c->head_rounds > 2 ? 2 : c->head_rounds);      // D = 256: 62 KB of LDS per te_head workgroup, two per CU
    // te_wgrad launches (output-tile jobs) x n_kc K-chunks: fill the CUs exactly (no ragged second round)
    const bool bt = poi::te_bintab(D, spatial, spatial ? P->n_dist : -1) && n >= c->bintab_min;
    const int jobs = poi::te_wgrad_jobs(D, spatial ? P->n_dist : -1, spatial, bt), nui = poi::te_wgrad_ui_jobs(D, spatial ? P->n_dist : -1, spatial, bt);
    n_kc = (c->num_cu * c->wgrad_rounds) / jobs;
    if (n_kc < 1) n_kc = 1;
    n_kc_ui = n_kc;
    if (bt && c->ppoi) {
      // per-POI regrouping: te_wgrad picks the K-chunk split on the device from the launch's own S-row count; the slabs are sized for
      // the extremes (no S rows: every slot goes to the T-row jobs; as many S rows as steps: the uniform split)
      int a, b;
      poi::te_wgrad_split(c->num_cu * c->wgrad_rounds, nui, jobs, 1, 1 << 20, &a, &b);
      n_kc_ui = n_kc;
      n_kc = a > n_kc ? a : n_kc;
      if ((rc = ensure(c, c->kc_dev, 64, st))) return rc;
    }
    n_slab = n_kc > n_kc_ui ? n_kc : n_kc_ui;
    if ((rc = ensure(c, c->hslab, sizeof(float) * (size_t)n_head * ((NB + 4) & ~3), st))) return rc;
  } else if ((rc = ensure(c, c->ws, sizeof(float) * wsf * grid, st))) return rc;
  if ((rc = ensure(c, c->slab, sizeof(float) * (size_t)dl.total * n_slab, st))) return rc;
  if (!tile && (rc = ensure(c, c->g_lt, sizeof(float) * (size_t)(P->n_item + 1) * D, st))) return rc;      // (10 GB at 10 M POIs x 256)
  if ((rc = ensure(c, c->mult_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if ((rc = ensure(c, c->nseq_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if (spatial) {
    if (!tile && (rc = ensure(c, c->g_di, sizeof(float) * (size_t)(P->n_dist + 1) * D, st))) return rc;
    if ((rc = ensure(c, c->mult_di, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
    if ((rc = ensure(c, c->nseq_di, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
  }
  poi::SeqArgs A;
  fill_args(A, P, T, uidx, n);
  const float bcap = c->batch_cap == 0.0f ? -(float)n : c->batch_cap;      // 0: mini-batch rule, encoded as -n (rule_scales)
  A.out = out; A.bcap = bcap;
  A.ws = (float*)c->ws.p; A.ws_stride = wsf;
  A.slab = (float*)c->slab.p;
  A.g_lt = (float*)c->g_lt.p; A.mult_lt = (int*)c->mult_lt.p; A.nseq_lt = (int*)c->nseq_lt.p;
  A.g_di = (float*)c->g_di.p; A.mult_di = (int*)c->mult_di.p; A.nseq_di = (int*)c->nseq_di.p;
  if (tile) {
    poi::TeArgs E;
    if ((rc = te_setup(c, E, P, T, uidx, n, false, spatial, st))) return rc;
    if ((rc = ensure(c, c->zrow, sizeof(float) * 1024, st))) return rc;
    E.zrow = (const float*)c->zrow.p;
    E.sr_salt = (c->f16_rounding && E.lt_f16) ? (++c->sr_counter) * 0x9E3779B1u | 1u : 0u;
    E.out = out; E.bcap = bcap; E.slab = A.slab; E.n_slab = n_slab; E.n_head = n_head; E.n_kc = n_kc; E.wg_slots = c->num_cu * c->wgrad_rounds;
    E.kc_dev = (E.bintab && c->ppoi) ? (int*)c->kc_dev.p : nullptr;
    E.hslab = (float*)c->hslab.p; E.hstride = (NB + 4) & ~3;
    E.side2 = c->side2; E.ev_h0 = c->ev_h0; E.ev_h1 = c->ev_h1; E.ev_h2 = c->ev_h2; E.ev_h3 = c->ev_h3;
    E.side = c->side; E.ev_slots = c->ev_slots; E.ev_sorted = c->ev_sorted; E.ev_bwd = c->ev_bwd; E.ev_fin = c->ev_fin; E.ev_start = c->ev_start; E.ev_pack = c->ev_pack;
    E.early_bins = (c->early_bins && E.bintab && c->side && n >= c->early_min) ? 1 : 0; E.bin_alpha = alpha; E.bin_lambda = lambda;
    E.dhot_on = (E.early_bins && E.ppoi && c->hot_bins) ? 1 : 0;
    E.hot_early = (c->hot_early && E.side && E.ppoi) ? 1 : 0; E.ev_hr0 = c->ev_hr0; E.ev_hr1 = c->ev_hr1;      // (ppoi: the hot rows' entries carry no per-entry dx rows - nothing te_gemm_dx produces is read)      // (te_dprep - the selection - must have run before te_psum: the early chain)
    E.mult_lt = A.mult_lt; E.nseq_lt = A.nseq_lt; E.mult_di = A.mult_di; E.nseq_di = A.nseq_di;
    A.kc_dev = E.kc_dev;                 // (dense_apply reads te_wgrad's K-chunk counts from the device)
    // one sequence (the reference schedule): the whole step in five kernels (tile_engine.hip, te_one_*)
    const bool one = n == 1 && c->one_path && E.rec1 && !E.lt_f16 && poi::te_one_supported(D, spatial, T->max_len);
    {
      poi_ctx::LastPlan& R = c->plan;
      R.tile = 1; R.one = one; R.rec1 = E.rec1; R.xrec1 = E.xrec1; R.hyb = E.hyb; R.bintab = E.bintab; R.ppoi = E.ppoi; R.listed = E.urow != nullptr;
      R.fwd_tab = E.fwd_tab; R.xft = E.xft; R.xcomp = E.xcomp; R.head_split = E.head_split; R.efuse = one ? 0 : E.efuse; R.early_bins = E.early_bins;
      R.hyb_dev = E.hyb_dev; R.st = st; R.ws_gen = c->te_ws_gen;      // (fork: launch_te_scatter)
    }
    // captured: a replay re-issues the launch id this launch got when it was captured - atomicMax against whatever a LATER launch left in xflag
    // would keep the newer id and lose this replay's NaN flag.  The captured sequence therefore starts by clearing the flag: only
    // its own pack kernels can raise it to its own id (they run behind ev_start, i.e. behind this node).
    bool captured = false;
    auto run = [&](hipStream_t s) -> hipError_t {
      if (captured && E.xflag) { hipError_t me = hipMemsetAsync(E.xflag, 0, sizeof(int), s); if (me != hipSuccess) return me; }
      if (one) { E.efuse = 0; return poi::launch_te_one(E, alpha, lambda, T->max_len, s, &c->tm); }
      hipError_t e = poi::launch_te_train(E, c->num_cu, s, &c->tm);
      // early distance-bin chain (launch_te_train started it on the side stream behind te_wgrad): the dense write-back needs te_wgrad's slabs,
      // te_finalize's parts and te_dui's - all of them older on the side stream - and nothing the POI rows' reduction on `s` reads: it
      // follows the chain there, and launch_te_scatter's join (ev_slots) waits for both
      const bool dense_side = E.early_bins && E.bintab && E.side;
      if (e == hipSuccess && dense_side) {
        e = poi::launch_dense_apply(A, spatial, n_slab, n_slab, alpha, lambda, E.side, &c->tm);
        if (e == hipSuccess) e = hipEventRecord(E.ev_slots, E.side);
      }
      if (e == hipSuccess) e = poi::launch_te_scatter(E, alpha, lambda, c->num_cu, s, &c->tm, &c->plan.fork);
      if (e == hipSuccess && !dense_side) e = poi::launch_dense_apply(A, spatial, n_slab, n_slab, alpha, lambda, s, &c->tm);
      return e;
    };
    const size_t out_bytes = sizeof(float) * (size_t)n * (spatial ? 5 : 1);
    // (timing: only the SAMPLED launches carry event pairs - the others replay; a sampled launch runs eagerly)
    if (!c->graph_mode || (c->tm.on && c->tm.active) || !c->side || n < c->graph_min_n || n > c->graph_max_n || E.sr_salt) { HIPCHK(c, run(st)); return POI_OK; }
    // ---- graph replay ----
    if ((rc = ensure(c, c->uidx_stage, sizeof(int32_t) * (size_t)n, st)) || (rc = ensure(c, c->out_stage, out_bytes, st))) return rc;
    std::vector<uint64_t> key;
    {
      auto add = [&](const void* p, size_t bytes) { const size_t w = (bytes + 7) / 8, o = key.size(); key.resize(o + w, 0); memcpy(key.data() + o, p, bytes); };
      add(P, sizeof *P); add(T, sizeof *T);
      const uint64_t sc[] = {(uint64_t)n, (uint64_t)spatial, (uint64_t)c->engine, (uint64_t)c->ppoi, (uint64_t)n_head, (uint64_t)n_kc, (uint64_t)n_slab,
                             (uint64_t)c->wgrad_rounds, (uint64_t)is_f16(c, P->lt)};
      (void)bcap;
      add(sc, sizeof sc);
      const float fs[] = {alpha, lambda, c->batch_cap, 0.f};
      add(fs, sizeof fs);
      const void* bufs[] = {c->te_ws.p, c->slab.p, c->hslab.p, c->zrow.p, c->seg_s.p, c->seg_e.p, c->pmark.p, c->xc.p, c->kc_dev.p, c->mult_lt.p, c->nseq_lt.p,
                            c->mult_di.p, c->nseq_di.p, c->uidx_stage.p, c->out_stage.p, c->ptab.p, c->iota.p, c->xw.p, c->xg.p, c->xflag.p};
      add(bufs, sizeof bufs);
      // every switch that decides which kernels / which stream topology the launch takes, each in its own word (packed into one
      // word they overlapped and early_min was missing), plus what te_setup derived from them for THIS launch
      const uint64_t sw[] = {(uint64_t)c->fwd_tab, (uint64_t)c->rec_split, (uint64_t)c->one_path, (uint64_t)(unsigned)c->rec1_max, (uint64_t)(unsigned)c->bintab_min,
                             (uint64_t)c->early_bins, (uint64_t)(unsigned)c->early_min, (uint64_t)c->xfwd, (uint64_t)E.early_bins, (uint64_t)E.bintab, (uint64_t)E.rec1,
                             (uint64_t)E.fwd_tab, (uint64_t)E.xfwd, (uint64_t)E.xft, (uint64_t)E.xrec1, (uint64_t)E.xcomp, (uint64_t)(unsigned)c->xcomp_min, (uint64_t)E.head_split, (uint64_t)(unsigned)c->xrec1_max, (uint64_t)E.ppoi, (uint64_t)one, (uint64_t)E.hyb, (uint64_t)E.efuse, (uint64_t)E.hot_early};
      add(sw, sizeof sw);
    }
    poi_ctx::StepGraph* g = nullptr;
    for (auto& e : c->graphs) if (e.key == key) { g = &e; break; }
    if (!g && c->seen_key != key) {       // first sight: run eagerly (first-use initialisation happens outside any capture)
      c->seen_key = key;
      HIPCHK(c, run(st));
      return POI_OK;
    }
    HIPCHK(c, hipMemcpyAsync(c->uidx_stage.p, uidx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (!g) {
      E.uidx = (const int32_t*)c->uidx_stage.p; E.out = (float*)c->out_stage.p;
      A.uidx = E.uidx; A.out = E.out;
      hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
      hipError_t e = hipStreamBeginCapture(c->cap, hipStreamCaptureModeRelaxed);
      if (e == hipSuccess) {
        captured = true;
        e = run(c->cap);
        captured = false;
        const hipError_t e2 = hipStreamEndCapture(c->cap, &graph);
        if (e == hipSuccess) e = e2;
      }
      if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        c->graph_mode = 0;                 // this runtime cannot capture the launch: stay eager
        E.uidx = uidx; E.out = out; A.uidx = uidx; A.out = out;
        HIPCHK(c, run(st));
        return POI_OK;
      }
      if (c->graphs.size() >= 8) {         // evict the least recently used
        size_t lru = 0;
        for (size_t i = 1; i < c->graphs.size(); ++i) if (c->graphs[i].stamp < c->graphs[lru].stamp) lru = i;
        HIPCHK(c, hipStreamSynchronize(st));
        (void)hipGraphExecDestroy(c->graphs[lru].exec); (void)hipGraphDestroy(c->graphs[lru].graph);
        c->graphs.erase(c->graphs.begin() + lru);
      }
      c->graphs.push_back(poi_ctx::StepGraph{key, graph, exec, 0, c->plan.fork});
      g = &c->graphs.back();
      ++c->graph_captures;
    }
    g->stamp = ++c->graph_stamp;
    c->plan.fork = g->fork;
    HIPCHK(c, hipGraphLaunch(g->exec, st));
    ++c->graph_replays;
    HIPCHK(c, hipMemcpyAsync(out, c->out_stage.p, out_bytes, hipMemcpyDeviceToDevice, st));
    return POI_OK;
  }
  HIPCHK(c, poi::launch_seq_train(A, spatial, grid, alpha, lambda, st, &c->tm));
  return POI_OK;
}

int poi_spatial_step(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n,
                     float alpha, float lambda, float* out, void* stream) {
  return seq_step(c, P, T, uidx, n, alpha, lambda, out, stream, true);
}

int poi_gru_step(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n,
                 float alpha, float lambda, float* out, void* stream) {
  return seq_step(c, P, T, uidx, n, alpha, lambda, out, stream, false);
}

int poi_gru_predict(poi_ctx* c, const poi_gru_params* P, const poi_seq_tables* T, const int32_t* uidx, const int32_t* out_row, int32_t n,
                    float* hts, float* sts, void* stream) {
  const bool spatial = P && P->di != nullptr;
  int rc = check_gru(c, P, T, spatial, false);
  if (rc) return rc;
  if (!uidx || !hts || n < 0) return fail(c, POI_EINVAL, "uidx/hts NULL or n < 0");
  if (n == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (use_tile(c, P, spatial, n)) {
    poi::TeArgs E;
    if ((rc = te_setup(c, E, P, T, uidx, n, true, spatial, (hipStream_t)stream))) return rc;
    E.hts = hts; E.sts = sts; E.out_row = out_row;
    HIPCHK(c, poi::launch_te_predict(E, c->num_cu, (hipStream_t)stream, &c->tm));
    return POI_OK;
  }
  if (is_f16(c, P->lt)) return fail(c, POI_ENOTSUP, "a half POI table needs the tile engine (dim 64 / 128 / 256, <= 2048 bins)");
  int grid = c->num_cu * c->wg_per_cu;
  if (grid > n) grid = n;
  if (c->engine == 4) {
    if (spatial && P->n_dist + 1 > 4096) return fail(c, POI_ENOTSUP, "the exact engine supports at most 4095 distance bins");
    poi::ExArgs X;
    fill_ex(X, P, T, uidx, n);
    X.hts = hts; X.sts = sts; X.out_row = out_row;
    HIPCHK(c, poi::launch_ex_predict(X, spatial, grid, (hipStream_t)stream, &c->tm));
    return POI_OK;
  }
  poi::SeqArgs A;
  fill_args(A, P, T, uidx, n);
  A.hts = hts; A.sts = sts; A.out_row = out_row;
  HIPCHK(c, poi::launch_seq_predict(A, spatial, grid, (hipStream_t)stream, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
static int check_carnn(poi_ctx* c, const poi_carnn_params* P, const poi_seq_tables* T, bool need_q) {
  if (!c || !P || !T) return fail(c, POI_EINVAL, "NULL ctx/params/tables");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "dim must be a multiple of 4 in [4, 256] (got %d)", P->dim);
  if (!P->lt || !P->wd || !P->M || P->n_dist <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "CA-RNN needs lt / wd / M, n_item > 0 and n_dist > 0");
  if (!T->off || !T->p || !T->dp) return fail(c, POI_EINVAL, "tables: off/p/dp must be non-NULL");
  if (need_q && (!T->q || !T->dq)) return fail(c, POI_EINVAL, "tables: q/dq must be non-NULL");
  if (T->max_len <= 0 || T->len_max < T->max_len) return fail(c, POI_EINVAL, "tables: need 0 < max_len <= len_max");
  return POI_OK;
}

static void fill_carnn(poi::CaArgs& A, const poi_carnn_params* P, const poi_seq_tables* T, const int32_t* uidx, int n) {
  memset(&A, 0, sizeof A);
  A.lt = P->lt; A.wd = P->wd; A.M = P->M; A.n_item = P->n_item; A.n_dist = P->n_dist; A.dim = P->dim;
  A.off = T->off; A.p = T->p; A.q = T->q; A.dp = T->dp; A.dq = T->dq; A.len_max = T->len_max; A.cap = T->max_len;
  A.uidx = uidx; A.n_seq = n; A.bcap = 1.0f;
}

int poi_carnn_step(poi_ctx* c, const poi_carnn_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n,
                   float alpha, float lambda, float* out, void* stream) {
  int rc = check_carnn(c, P, T, true);
  if (rc) return rc;
  if (is_f16(c, P->lt)) return fail(c, POI_ENOTSUP, "CA-RNN supports float32 tables only");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (!uidx || !out || n < 0) return fail(c, POI_EINVAL, "uidx/out NULL or n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  const int D = P->dim;
  const bool fast = c->carnn_fast && (D == 64 || D == 128) && P->n_dist + 2 <= 2048;
  int grid = c->num_cu * (fast ? (getenv("POI_SEQ_WG_PER_CU") ? c->wg_per_cu : 8) : c->wg_per_cu);
  if (grid > n) grid = n;
  const size_t wsf = poi::carnn_ws_floats(D, T->max_len);
  if ((rc = ensure(c, c->ca_ws, sizeof(float) * wsf * grid, st))) return rc;
  if ((rc = ensure(c, c->ca_slab, sizeof(float) * (size_t)D * D * grid, st))) return rc;
  if ((rc = ensure(c, c->g_lt, sizeof(float) * (size_t)(P->n_item + 1) * D, st))) return rc;
  if ((rc = ensure(c, c->mult_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if ((rc = ensure(c, c->nseq_lt, sizeof(int) * (size_t)(P->n_item + 1), st))) return rc;
  if ((rc = ensure(c, c->g_wd, sizeof(float) * (size_t)(P->n_dist + 1) * D * D, st))) return rc;
  if ((rc = ensure(c, c->mult_wd, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
  if ((rc = ensure(c, c->nseq_wd, sizeof(int) * (size_t)(P->n_dist + 1), st))) return rc;
  poi::CaArgs A;
  fill_carnn(A, P, T, uidx, n);
  A.out = out; A.bcap = c->batch_cap;
  A.ws = (float*)c->ca_ws.p; A.ws_stride = wsf; A.slab = (float*)c->ca_slab.p;
  A.g_lt = (float*)c->g_lt.p; A.mult_lt = (int*)c->mult_lt.p; A.nseq_lt = (int*)c->nseq_lt.p;
  A.g_wd = (float*)c->g_wd.p; A.mult_wd = (int*)c->mult_wd.p; A.nseq_wd = (int*)c->nseq_wd.p;
  if (fast) {
    // (the recurrence kernel is bound by the L2 stream of the interval matrices: eight workgroups per CU instead of two, +29 %)
    // outer-product path (carnn.hip): packed per-step state + sorted entries, matrix gradients on the matrix cores
    const size_t Tcap = (size_t)n * (size_t)(T->max_len > 1 ? T->max_len - 1 : 1), Ne = 6 * Tcap, NK = (size_t)P->n_dist + 2;
    const size_t n_chunk = Ne / 512 + NK + 1;
    const size_t N2 = 3 * Tcap;
    const size_t nint = (size_t)n + 8 + 6 * Ne + (size_t)RS_HIST_INTS + RS_MAXBIN + 16 + 3 * (NK + 8) + 4 * N2 + 2 * ((size_t)P->n_item + 8) + 32;
    const size_t nfl = (Tcap + (size_t)n + 1) * D + Tcap * 5 * D + n_chunk * (size_t)D * D + ((size_t)P->n_item + 4) * D + N2 * D + 64;
    if ((rc = ensure(c, c->ca2, 4 * (nint + nfl) + 256, st))) return rc;
    float* f = (float*)c->ca2.p;
    auto take = [&](size_t cnt) { float* r = f; f += (cnt + 3) & ~(size_t)3; return r; };
    A.Hpk = take((Tcap + (size_t)n + 1) * D); A.EA = take(Tcap * 5 * D); A.partial = take(n_chunk * (size_t)D * D);
    A.PM = take(((size_t)P->n_item + 2) * D);
    A.vpart = take(N2 * D);
    if (n < 16) A.PM = nullptr;      // a handful of sequences: three GEMVs per step are cheaper than the table (measured: a wash at one)
    int* ip = (int*)f;
    auto itake = [&](size_t cnt) { int* r = ip; ip += (cnt + 3) & ~(size_t)3; return r; };
    A.soff = itake((size_t)n + 1); A.keys0 = itake(Ne); A.keys1 = itake(Ne); A.vals0 = itake(Ne); A.vals1 = itake(Ne);
    A.ent_a = itake(Ne); A.ent_b = itake(Ne); A.hist = itake((size_t)RS_HIST_INTS + RS_MAXBIN); A.cnt = itake(8);
    A.seg_start = itake(NK + 4); A.seg_end = itake(NK + 4); A.chunk_first = itake(NK + 4);
    A.k2a = itake(N2); A.k2b = itake(N2); A.v2a = itake(N2); A.v2b = itake(N2);
    A.seg2_start = itake((size_t)P->n_item + 4); A.seg2_end = itake((size_t)P->n_item + 4);
    A.n_chunk_cap = (int)n_chunk;
    HIPCHK(c, poi::launch_carnn_train2(A, grid, alpha, lambda, st, &c->tm));
    return POI_OK;
  }
  HIPCHK(c, poi::launch_carnn_train(A, grid, alpha, lambda, st, &c->tm));
  return POI_OK;
}

int poi_carnn_predict(poi_ctx* c, const poi_carnn_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n, float* hts, void* stream) {
  int rc = check_carnn(c, P, T, false);
  if (rc) return rc;
  if (!uidx || !hts || n < 0) return fail(c, POI_EINVAL, "uidx/hts NULL or n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->ca_scr, sizeof(float) * ((size_t)(P->n_dist + 1) * P->dim + (size_t)P->n_item + 2048), st))) return rc;
  poi::CaArgs A;
  fill_carnn(A, P, T, uidx, n);
  A.hts = hts;
  int grid = c->num_cu * 4;
  if (grid > n) grid = n;
  HIPCHK(c, poi::launch_carnn_predict(A, grid, (float*)c->ca_scr.p, st, &c->tm));
  return POI_OK;
}

int poi_carnn_score_all(poi_ctx* c, const float* users, const float* items, const float* M, const float* dists, const double* coords,
                        const double* cphi, const double* thr, const int32_t* last_poi, int32_t n, int32_t n_item, int32_t n_dist, int32_t dim,
                        double dd, float* scores_out, void* stream) {
  if (!c || !users || !items || !M || !dists || !coords || !cphi || !thr || !last_poi || !scores_out) return fail(c, POI_EINVAL, "poi_carnn_score_all: NULL argument");
  if (n < 0 || n_item <= 0 || n_dist <= 0 || dim <= 0 || !(dd > 0)) return fail(c, POI_EINVAL, "bad sizes");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->ca_scr, sizeof(float) * ((size_t)(n_dist + 1) * dim + (size_t)n_item + 2048), st))) return rc;
  for (int32_t o = 0; o < n; o += 32768) {
    const int32_t m = n - o < 32768 ? n - o : 32768;
    HIPCHK(c, poi::launch_carnn_score(users + (size_t)o * dim, items, M, dists, coords, cphi, thr, last_poi + o, m, n_item, n_dist, dim, dd,
                                      (float*)c->ca_scr.p, scores_out + (size_t)o * n_item, st, &c->tm));
  }
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
int poi_bpr_step(poi_ctx* c, float* ux, float* lt, int32_t n_user, int32_t n_item, int32_t dim,
                 const int32_t* uidx, const int32_t* p, const int32_t* q, int32_t n,
                 float alpha, float lambda, float* loss_out, int mode, void* stream) {
  if (!c || !ux || !lt || !uidx || !p || !q || !loss_out) return fail(c, POI_EINVAL, "poi_bpr_step: NULL argument");
  if (is_f16(c, ux)) return fail(c, POI_ENOTSUP, "BPR-MF keeps the user table in float32 (a half POI table is supported in snapshot mode)");
  if (is_f16(c, lt) && mode != POI_BPR_SNAPSHOT) return fail(c, POI_ENOTSUP, "a half POI table needs POI_BPR_SNAPSHOT");
  if (dim <= 0 || dim % 4 != 0 || dim > 1024) return fail(c, POI_ENOTSUP, "dim must be a multiple of 4 in [4, 1024] (got %d)", dim);
  if (n < 0 || n_user <= 0 || n_item <= 0) return fail(c, POI_EINVAL, "bad sizes");
  if ((int64_t)n * 3 >= (int64_t)1 << 31) return fail(c, POI_ENOTSUP, "at most 2^31 / 3 triples per launch");
  if (mode != POI_BPR_SNAPSHOT && mode != POI_BPR_HOGWILD) return fail(c, POI_EINVAL, "unknown mode %d", mode);
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::BprArgs A;
  memset(&A, 0, sizeof A);
  A.ux = ux; A.lt = lt; A.n_user = n_user; A.n_item = n_item; A.dim = dim;
  A.lt_f16 = is_f16(c, lt);
  A.sr_salt = (c->f16_rounding && A.lt_f16) ? (++c->sr_counter) * 0x9E3779B1u | 1u : 0u;
  A.uidx = uidx; A.p = p; A.q = q; A.n = n; A.alpha = alpha; A.lambda = lambda; A.loss = loss_out; A.bcap = c->batch_cap;
  { int rc0 = ensure(c, c->bad_ids, 64, st); if (rc0) return rc0; }      // (zero-filled at allocation)
  A.bad = (int*)c->bad_ids.p;
  if (mode == POI_BPR_SNAPSHOT) {
    // workspace: the 3 n touches' sort buffers, per-triple coefficients, per-window partial sums; the shadow user table (grow-only, ctx-owned)
    int rc;
    size_t ni = 0, nf = 0;
    poi::bpr_ws_sizes(n, dim, &ni, &nf);
    if ((rc = ensure(c, c->g_ux, sizeof(float) * (size_t)n_user * dim, st))) return rc;
    if ((rc = ensure(c, c->g_blt, sizeof(int) * ni + sizeof(float) * nf + 256, st))) return rc;
    A.shadow = (float*)c->g_ux.p;
    const size_t chunks = (size_t)(n + 63) / 64 + (size_t)(2 * (size_t)n + 63) / 64 + 2, per = 3 * (size_t)n + 64;
    int* ip = (int*)c->g_blt.p;
    A.keys0 = ip; A.keys1 = ip + per; A.vals0 = ip + 2 * per; A.vals1 = ip + 3 * per; ip += 4 * per;
    A.hist = ip; ip += RS_HIST_INTS + RS_MAXBIN;
    A.cnt = ip; ip += 64;
    A.meta = (int4*)ip; ip += 4 * chunks;
    float* fp = (float*)ip;
    A.g = fp; fp += ((size_t)n + 64 + 3) & ~(size_t)3;      // (lead / trail rows are read as float4)
    A.lead = fp; fp += chunks * (size_t)dim;
    A.trail = fp;
  }
  HIPCHK(c, poi::launch_bpr(A, mode, c->num_cu, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// VBPR (vbpr.hip)
static int vbpr_check(poi_ctx* c, const poi_vbpr_params* P, const char* who, poi::VbprArgs& A) {
  if (!c || !P) return fail(c, POI_EINVAL, "%s: NULL ctx/params", who);
  if (!P->ux || !P->lt || !P->ue || !P->ei || !P->fi) return fail(c, POI_EINVAL, "%s: ux/lt/ue/ei/fi must be non-NULL", who);
  if (is_f16(c, P->ux) || is_f16(c, P->lt) || is_f16(c, P->ue) || is_f16(c, P->ei) || is_f16(c, P->fi)) return fail(c, POI_ENOTSUP, "VBPR tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "VBPR: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->n_img <= 0 || P->n_img % 4 != 0 || P->n_img > 4096) return fail(c, POI_ENOTSUP, "VBPR: n_img must be a multiple of 4 in [4, 4096] (got %d)", P->n_img);
  if (((uintptr_t)P->fi | (uintptr_t)P->ei | (uintptr_t)P->ux | (uintptr_t)P->ue | (uintptr_t)P->lt) & 15) return fail(c, POI_EINVAL, "%s: the tables must be 16-byte aligned", who);
  if (P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "%s: bad sizes", who);
  if (2 * (int64_t)P->n_user + (int64_t)P->n_item + 1 >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "VBPR: 2 n_user + n_item + 1 must stay below 2^31");
  memset(&A, 0, sizeof A);
  A.ux = P->ux; A.lt = P->lt; A.ue = P->ue; A.ei = P->ei; A.fi = P->fi;
  A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim; A.n_img = P->n_img;
  A.sentinel = 2 * P->n_user + P->n_item + 1;
  A.grid_cap = c->vbpr_grid;
  return POI_OK;
}

int poi_vbpr_step(poi_ctx* c, const poi_vbpr_params* P, const int32_t* uidx, const int32_t* p, const int32_t* q, int32_t n, float alpha,
                  float lambda, float lambda_ev, float* loss_out, void* stream) {
  poi::VbprArgs A;
  int rc = vbpr_check(c, P, "poi_vbpr_step", A);
  if (rc) return rc;
  if (!uidx || !p || !q || !loss_out) return fail(c, POI_EINVAL, "poi_vbpr_step: NULL argument");
  if (n < 0) return fail(c, POI_EINVAL, "poi_vbpr_step: bad sizes");
  if ((int64_t)n * 4 >= ((int64_t)1 << 31) - 64) return fail(c, POI_ENOTSUP, "VBPR: at most 2^31 / 4 triples per launch");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  A.uidx = uidx; A.p = p; A.q = q; A.n = n; A.alpha = alpha; A.lambda = lambda; A.lambda_ev = lambda_ev; A.bcap = c->batch_cap; A.loss = loss_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  poi::vbpr_chunking(n, &A.ch_rows, &A.n_chunk);
  size_t ni = 0, nf = 0, nd = 0;
  poi::vbpr_ws_sizes(n, P->dim, P->n_img, &ni, &nf, &nd);
  if ((rc = ensure(c, c->vb_ws, sizeof(double) * nd + sizeof(int) * ni + sizeof(float) * nf + 512, st))) return rc;
  const size_t chunks = ((size_t)4 * n + 63) / 64 + 2, per = 4 * (size_t)n + 64, nt = ((size_t)n + 64 + 3) & ~(size_t)3;
  A.dpart = (double*)c->vb_ws.p;
  int* ip = (int*)(A.dpart + ((nd + 1) & ~(size_t)1));      // (16-byte aligned behind the float64 partials)
  A.keys0 = ip; A.keys1 = ip + per; A.vals0 = ip + 2 * per; A.vals1 = ip + 3 * per; ip += 4 * per;
  A.hist = ip; ip += RS_HIST_INTS + RS_MAXBIN;
  A.cnt = ip; ip += 64;
  A.meta = (int4*)ip; ip += 4 * chunks;
  A.okf = ip; ip += nt;
  A.ord = ip; ip += nt;
  float* fp = (float*)ip;
  A.g = fp; fp += nt;
  A.V = fp; fp += (size_t)n * P->dim;
  A.lead = fp; fp += chunks * (size_t)P->dim;
  A.trail = fp; fp += chunks * (size_t)P->dim;
  A.slot = fp;
  HIPCHK(c, poi::launch_vbpr_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

int poi_vbpr_items(poi_ctx* c, const poi_vbpr_params* P, float* items_out, void* stream) {
  poi::VbprArgs A;
  int rc = vbpr_check(c, P, "poi_vbpr_items", A);
  if (rc) return rc;
  if (!items_out) return fail(c, POI_EINVAL, "poi_vbpr_items: NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  A.out = items_out; A.n_rows = P->n_item + 1;
  HIPCHK(c, poi::launch_vbpr_items(A, c->num_cu, (hipStream_t)stream, &c->tm));
  return POI_OK;
}

int poi_vbpr_users(poi_ctx* c, const poi_vbpr_params* P, float* users_out, void* stream) {
  poi::VbprArgs A;
  int rc = vbpr_check(c, P, "poi_vbpr_users", A);
  if (rc) return rc;
  if (!users_out) return fail(c, POI_EINVAL, "poi_vbpr_users: NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_vbpr_users(P->ux, P->ue, P->n_user, P->dim, users_out, c->num_cu, (hipStream_t)stream, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// FPMC-LR (fpmc.hip)
// c >= (1 - cos a) / 2 = sin^2(a / 2): a POI more than 2 asin(sqrt(c)) away in latitude is never within the radius (1e-6 relative margin)
static double lat_band_deg(double c) { return c >= 1.0 ? 1e9 : 2.0 * asin(sqrt(c)) / 0.017453292519943295 * (1.0 + 1e-6) + 1e-9; }

static int fpmc_nbr_common(poi_ctx* c, const double* coords, const double* cphi, const int32_t* lat_order, int32_t n_item, double c_ud,
                           const char* who, poi::FpmcNbrArgs& A) {
  if (!c || !coords || !cphi || !lat_order) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (n_item <= 0) return fail(c, POI_EINVAL, "%s: n_item must be positive (got %d)", who, n_item);
  if (!(c_ud >= 0.0)) return fail(c, POI_EINVAL, "%s: c_ud must be >= 0", who);
  memset(&A, 0, sizeof A);
  A.coords = coords; A.cphi = cphi; A.order = lat_order; A.n = n_item; A.c_ud = c_ud;
  A.band_deg = lat_band_deg(c_ud);
  return POI_OK;
}

int poi_fpmc_neighbor_counts(poi_ctx* c, const double* coords, const double* cphi, const int32_t* lat_order, int32_t n_item, double c_ud,
                             int64_t* off_out, void* stream) {
  poi::FpmcNbrArgs A;
  int rc = fpmc_nbr_common(c, coords, cphi, lat_order, n_item, c_ud, "poi_fpmc_neighbor_counts", A);
  if (rc) return rc;
  if (!off_out) return fail(c, POI_EINVAL, "poi_fpmc_neighbor_counts: NULL argument");
  A.off = (long long*)off_out;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("fpmc_nbr_count", (hipStream_t)stream);
  HIPCHK(c, poi::launch_fpmc_neighbors(A, 0, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_fpmc_neighbor_fill(poi_ctx* c, const double* coords, const double* cphi, const int32_t* lat_order, int32_t n_item, double c_ud,
                           const int64_t* off, int32_t* nbr_out, void* stream) {
  poi::FpmcNbrArgs A;
  int rc = fpmc_nbr_common(c, coords, cphi, lat_order, n_item, c_ud, "poi_fpmc_neighbor_fill", A);
  if (rc) return rc;
  if (!off || !nbr_out) return fail(c, POI_EINVAL, "poi_fpmc_neighbor_fill: NULL argument");
  A.off = (long long*)off; A.nbr = nbr_out;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("fpmc_nbr_fill", (hipStream_t)stream);
  HIPCHK(c, poi::launch_fpmc_neighbors(A, 1, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_fpmc_sample_negatives(poi_ctx* c, const int64_t* nbr_off, const int32_t* nbr, int32_t n_item, const int32_t* pos, int64_t n, uint64_t seed,
                              int32_t* neg_out, void* stream) {
  if (!c || !nbr_off || !nbr || !pos || !neg_out) return fail(c, POI_EINVAL, "poi_fpmc_sample_negatives: NULL argument");
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "poi_fpmc_sample_negatives: bad sizes");
  if (n == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("fpmc_sample", (hipStream_t)stream);
  HIPCHK(c, poi::launch_fpmc_sample((const long long*)nbr_off, nbr, pos, n, n_item, seed, neg_out, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_fpmc_step(poi_ctx* c, const poi_fpmc_params* P, const int32_t* u, const int32_t* a, const int32_t* i, const int32_t* j, int32_t n,
                  float alpha, float lambda, float* loss_out, void* stream) {
  if (!c || !P || !P->ui || !P->iu || !P->ia || !P->ai || !u || !a || !i || !j || !loss_out) return fail(c, POI_EINVAL, "poi_fpmc_step: NULL argument");
  if (is_f16(c, P->ui) || is_f16(c, P->iu) || is_f16(c, P->ia) || is_f16(c, P->ai)) return fail(c, POI_ENOTSUP, "FPMC-LR tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "FPMC-LR: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (n < 0 || P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "poi_fpmc_step: bad sizes");
  if ((int64_t)P->n_user + 3 * ((int64_t)P->n_item + 1) >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "FPMC-LR: n_user + 3 (n_item + 1) must stay below 2^31");
  if ((int64_t)n * 6 >= ((int64_t)1 << 31) - 64) return fail(c, POI_ENOTSUP, "FPMC-LR: at most 2^31 / 6 transitions per launch");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::FpmcArgs A;
  memset(&A, 0, sizeof A);
  A.ui = P->ui; A.iu = P->iu; A.ia = P->ia; A.ai = P->ai; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim;
  A.u = u; A.a = a; A.i = i; A.j = j; A.n = n; A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.loss = loss_out;
  A.sentinel = P->n_user + 3 * (P->n_item + 1);
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  size_t ni = 0, nf = 0;
  poi::fpmc_ws_sizes(n, P->dim, &ni, &nf);
  if ((rc = ensure(c, c->fp_ws, sizeof(int) * ni + sizeof(float) * nf + 256, st))) return rc;
  const size_t chunks = ((size_t)6 * n + 63) / 64 + 2, per = 6 * (size_t)n + 64;
  int* ip = (int*)c->fp_ws.p;
  A.keys0 = ip; A.keys1 = ip + per; A.vals0 = ip + 2 * per; A.vals1 = ip + 3 * per; ip += 4 * per;
  A.hist = ip; ip += RS_HIST_INTS + RS_MAXBIN;
  A.cnt = ip; ip += 64;
  A.meta = (int4*)ip; ip += 4 * chunks;
  float* fp = (float*)ip;
  A.s = fp; fp += ((size_t)n + 64 + 3) & ~(size_t)3;
  A.lead = fp; fp += chunks * (size_t)P->dim;
  A.trail = fp; fp += chunks * (size_t)P->dim;
  A.slot = fp;
  HIPCHK(c, poi::launch_fpmc_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// PRME (prme.hip)
static int prme_check(poi_ctx* c, const poi_prme_params* P, const char* who) {
  if (!c || !P || !P->du || !P->dp || !P->ds) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->du) || is_f16(c, P->dp) || is_f16(c, P->ds)) return fail(c, POI_ENOTSUP, "PRME tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "PRME: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "%s: bad sizes", who);
  return POI_OK;
}

int poi_prme_step(poi_ctx* c, const poi_prme_params* P, const int32_t* u, const int32_t* p, const int32_t* q, const int32_t* prev,
                  const double* d, const int32_t* gap, int32_t n, float alpha, float lambda, int32_t threshold, float cw, float* loss_out,
                  void* stream) {
  int rc = prme_check(c, P, "poi_prme_step");
  if (rc) return rc;
  if (!u || !p || !q || !prev || !d || !gap || !loss_out) return fail(c, POI_EINVAL, "poi_prme_step: NULL argument");
  if (n < 0) return fail(c, POI_EINVAL, "poi_prme_step: bad sizes");
  if ((int64_t)P->n_user + 2 * ((int64_t)P->n_item + 1) >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "PRME: n_user + 2 (n_item + 1) must stay below 2^31");
  if ((int64_t)n * 7 >= ((int64_t)1 << 31) - 64) return fail(c, POI_ENOTSUP, "PRME: at most 2^31 / 7 transitions per launch");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::PrmeArgs A;
  memset(&A, 0, sizeof A);
  A.du = P->du; A.dp = P->dp; A.ds = P->ds; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim;
  A.u = u; A.p = p; A.q = q; A.prev = prev; A.d = d; A.gap = gap; A.n = n; A.thd = threshold;
  A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.cw = cw; A.loss = loss_out;
  A.sentinel = P->n_user + 2 * (P->n_item + 1);
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  size_t ni = 0, nf = 0;
  poi::prme_ws_sizes(n, P->dim, &ni, &nf);
  if ((rc = ensure(c, c->pr_ws, sizeof(int) * ni + sizeof(float) * nf + 256, st))) return rc;
  const size_t chunks = ((size_t)7 * n + 63) / 64 + 2, per = 7 * (size_t)n + 64, nt = ((size_t)n + 64 + 3) & ~(size_t)3;
  int* ip = (int*)c->pr_ws.p;
  A.keys0 = ip; A.keys1 = ip + per; A.vals0 = ip + 2 * per; A.vals1 = ip + 3 * per; ip += 4 * per;
  A.hist = ip; ip += RS_HIST_INTS + RS_MAXBIN;
  A.cnt = ip; ip += 64;
  A.meta = (int4*)ip; ip += 4 * chunks;
  float* fp = (float*)ip;
  A.ga = fp; fp += nt;
  A.gb = fp; fp += nt;
  A.lead = fp; fp += chunks * (size_t)P->dim;
  A.trail = fp; fp += chunks * (size_t)P->dim;
  A.slot = fp;
  HIPCHK(c, poi::launch_prme_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

static int prme_score_common(poi_ctx* c, const poi_prme_params* P, const double* coords, const int32_t* users, const int32_t* qpoi, int32_t n_rows,
                             float cw, int32_t k, float* out, int32_t* idx_out, float* score_out, void* stream) {
  const char* who = k > 0 ? "poi_prme_score_topk" : "poi_prme_score_all";
  int rc = prme_check(c, P, who);
  if (rc) return rc;
  if (!coords || !users || !qpoi || (k > 0 ? !idx_out : !out)) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (n_rows < 0) return fail(c, POI_EINVAL, "%s: n_rows < 0", who);
  if (k > 0 && (k > 64 || k > P->n_item)) return fail(c, POI_EINVAL, "%s: k must lie in [1, min(64, n_item)] (got %d)", who, k);
  if (n_rows == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::PrmeScoreArgs A;
  memset(&A, 0, sizeof A);
  A.du = P->du; A.dp = P->dp; A.ds = P->ds; A.coords = coords; A.users = users; A.qpoi = qpoi;
  A.n_rows = n_rows; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim; A.k = k > 0 ? k : 0; A.cw = cw;
  A.out = out; A.idx_out = idx_out; A.sc_out = score_out;
  c->tm.begin(k > 0 ? "prme_score_topk" : "prme_score_all", st);
  HIPCHK(c, poi::launch_prme_score(A, st));
  c->tm.end(st);
  return POI_OK;
}

int poi_prme_score_all(poi_ctx* c, const poi_prme_params* P, const double* coords, const int32_t* users, const int32_t* qpoi, int32_t n_rows,
                       float cw, float* out, void* stream) {
  return prme_score_common(c, P, coords, users, qpoi, n_rows, cw, 0, out, nullptr, nullptr, stream);
}

int poi_prme_score_topk(poi_ctx* c, const poi_prme_params* P, const double* coords, const int32_t* users, const int32_t* qpoi,
                        int32_t n_rows, float cw, int32_t k, int32_t* idx_out, float* score_out, void* stream) {
  if (k <= 0) return fail(c, POI_EINVAL, "poi_prme_score_topk: k must be positive (got %d)", k);
  return prme_score_common(c, P, coords, users, qpoi, n_rows, cw, k, nullptr, idx_out, score_out, stream);
}

// ---------------------------------------------------------------------------------------------
// GeoIE (geoie.hip)
static int geoie_check(poi_ctx* c, const poi_geoie_params* P, const char* who) {
  if (!c || !P || !P->g || !P->h || !P->t || !P->z || !P->ab) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->g) || is_f16(c, P->h) || is_f16(c, P->t) || is_f16(c, P->z)) return fail(c, POI_ENOTSUP, "GeoIE tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "GeoIE: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "%s: bad sizes", who);
  return POI_OK;
}

// carve the GeoIE workspace for a launch of n users and P rows (256-byte aligned pieces); pairs: also the pair offsets
static int geoie_workspace(poi_ctx* c, poi::GeoieArgs& A, int n, int P, int dim, bool pairs, hipStream_t st) {
  const size_t chunks = ((size_t)5 * P + 63) / 64 + 2, T = 5 * (size_t)P + 64;
  const size_t sizes[] = {
      sizeof(int) * ((size_t)n + 1), sizeof(int) * ((size_t)n + 1), sizeof(int) * ((size_t)n + 1), sizeof(long long) * ((size_t)n + 1),
      sizeof(int) * ((size_t)n + 1), sizeof(int) * 8, sizeof(int) * ((size_t)P + 1), sizeof(float) * ((size_t)P + 1),
      sizeof(double) * ((size_t)P + 1) * 3, sizeof(double) * ((size_t)n + 1) * 2, pairs ? 0 : sizeof(float) * 3 * (size_t)P * dim,
      pairs ? 0 : sizeof(int) * T * 4, sizeof(int) * ((size_t)RS_HIST_INTS + RS_MAXBIN + 64), pairs ? 0 : sizeof(int4) * chunks * 2,
      pairs ? 0 : sizeof(float) * chunks * dim * 2, pairs ? 0 : sizeof(float) * 5 * (size_t)P * dim};
  size_t total = 0;
  for (size_t s : sizes) total += (s + 255) & ~(size_t)255;
  int rc = ensure(c, c->ge_ws, total + 256, st);
  if (rc) return rc;
  char* b = (char*)c->ge_ws.p;
  size_t i = 0;
  auto take = [&]() { char* r = b; b += (sizes[i++] + 255) & ~(size_t)255; return (void*)r; };
  A.rowoff = (int*)take(); A.troff = (int*)take(); A.tcoff = (int*)take(); A.pairoff = (long long*)take();
  A.ubad = (int*)take(); A.tot = (int*)take(); A.tuser = (int*)take(); A.coef = (float*)take();
  A.rloss = (double*)take(); A.rda = A.rloss + (P + 1); A.rdb = A.rda + (P + 1);
  A.uda = (double*)take(); A.udb = A.uda + (n + 1);
  A.G = (float*)take();
  int* kv = (int*)take();
  A.keys0 = kv; A.keys1 = kv + T; A.vals0 = kv + 2 * T; A.vals1 = kv + 3 * T;
  int* hc = (int*)take();
  A.hist = hc; A.cnt = hc + RS_HIST_INTS + RS_MAXBIN;
  A.meta = (int4*)take(); A.meta2 = A.meta + chunks;
  A.lead = (float*)take(); A.trail = A.lead + chunks * dim;
  A.slot = (float*)take();
  if (!pairs) A.pairoff = nullptr;
  return POI_OK;
}

int poi_geoie_step(poi_ctx* c, const poi_geoie_params* P, const int32_t* off, const int32_t* p, const int32_t* q, const double* coords,
                   const double* cphi, const int32_t* users, int32_t n, int64_t n_rows, float alpha, float lambda, double d_min,
                   float* loss_out, void* stream) {
  int rc = geoie_check(c, P, "poi_geoie_step");
  if (rc) return rc;
  if (!off || !p || !q || !coords || !cphi || !users || !loss_out) return fail(c, POI_EINVAL, "poi_geoie_step: NULL argument");
  if (n < 0 || n_rows < 0) return fail(c, POI_EINVAL, "poi_geoie_step: bad sizes");
  if (!(d_min >= 0.0)) return fail(c, POI_EINVAL, "poi_geoie_step: d_min must be >= 0");
  if (3 * ((int64_t)P->n_item + 1) >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "GeoIE: 3 (n_item + 1) must stay below 2^31");
  if (n_rows * 5 >= ((int64_t)1 << 31) - 64) return fail(c, POI_ENOTSUP, "GeoIE: at most 2^31 / 5 rows per launch");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::GeoieArgs A;
  memset(&A, 0, sizeof A);
  A.g = P->g; A.h = P->h; A.t = P->t; A.z = P->z; A.ab = P->ab; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim;
  A.off = off; A.p = p; A.q = q; A.users = users; A.coords = coords; A.cphi = cphi;
  A.n = n; A.P = (int)n_rows; A.n_pairs = -1; A.d_min = d_min;
  A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.loss = loss_out;
  A.sentinel = 3 * (P->n_item + 1);
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  if ((rc = geoie_workspace(c, A, n, (int)n_rows, P->dim, false, st))) return rc;
  HIPCHK(c, poi::launch_geoie_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

int poi_geoie_pair_distances(poi_ctx* c, const int32_t* off, const int32_t* p, const int32_t* q, int32_t n_user, int32_t n_item,
                             const double* coords, const double* cphi, const int32_t* users, int32_t n, int64_t n_rows, int64_t n_pairs,
                             float* dp_out, float* dq_out, void* stream) {
  if (!c || !off || !p || !q || !coords || !cphi || !users || !dp_out || !dq_out) return fail(c, POI_EINVAL, "poi_geoie_pair_distances: NULL argument");
  if (n < 0 || n_rows < 0 || n_pairs < 0 || n_user <= 0 || n_item <= 0 || n_rows >= ((int64_t)1 << 31) / 5)
    return fail(c, POI_EINVAL, "poi_geoie_pair_distances: bad sizes");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::GeoieArgs A;
  memset(&A, 0, sizeof A);
  A.n_user = n_user; A.n_item = n_item; A.off = off; A.p = p; A.q = q; A.users = users; A.coords = coords; A.cphi = cphi;
  A.n = n; A.P = (int)n_rows; A.n_pairs = n_pairs; A.dp_out = dp_out; A.dq_out = dq_out;
  int rc = geoie_workspace(c, A, n, (int)n_rows, 4, true, st);
  if (rc) return rc;
  c->tm.begin("geoie_pairs", st);
  HIPCHK(c, poi::launch_geoie_pairs(A, c->num_cu, st));
  c->tm.end(st);
  return POI_OK;
}

int poi_geoie_user_vectors(poi_ctx* c, const poi_geoie_params* P, const int32_t* off, const int32_t* p, int32_t n_user, int32_t len_max,
                           int32_t norm, float* out, void* stream) {
  int rc = geoie_check(c, P, "poi_geoie_user_vectors");
  if (rc) return rc;
  if (!off || !p || !out) return fail(c, POI_EINVAL, "poi_geoie_user_vectors: NULL argument");
  if (n_user < 0 || n_user > P->n_user || len_max < 0) return fail(c, POI_EINVAL, "poi_geoie_user_vectors: bad sizes");
  if (norm != 0 && norm != 1) return fail(c, POI_EINVAL, "poi_geoie_user_vectors: norm must be 0 (reference) or 1 (count)");
  if (n_user == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("geoie_uvec", st);
  HIPCHK(c, poi::launch_geoie_uvec(P->g, P->t, off, p, n_user, P->n_item, P->dim, len_max, norm, out, c->num_cu, st));
  c->tm.end(st);
  return POI_OK;
}

// scoring under the trained rule (geoie_score.hip): k == 0 writes the (n_rows, n_item) matrix, k > 0 the lists
static int geoie_score_common(poi_ctx* c, const char* who, const poi_geoie_params* P, const int32_t* off, const int32_t* p, const int32_t* mult,
                              const float* tu, const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min,
                              float* out, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out,
                              int32_t* count_out, void* stream) {
  int rc = geoie_check(c, P, who);
  if (rc) return rc;
  if (n_rows < 0) return fail(c, POI_EINVAL, "%s: n_rows < 0", who);
  if (!(d_min >= 0.0)) return fail(c, POI_EINVAL, "%s: d_min must be >= 0", who);
  if ((ex_off == nullptr) != (ex == nullptr)) return fail(c, POI_EINVAL, "%s: ex_off and ex go together", who);
  if (tu && is_f16(c, tu)) return fail(c, POI_ENOTSUP, "%s: tu must be float32", who);
  if (n_rows == 0) return POI_OK;
  if (!off || !p || !coords || !cphi) return fail(c, POI_EINVAL, "%s: NULL off / p / coords / cphi", who);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::GeoScoreArgs A = {};
  A.g = P->g; A.h = P->h; A.z = P->z; A.ab = P->ab; A.n_item = P->n_item; A.dim = P->dim;
  A.off = off; A.p = p; A.mult = mult; A.rows = rows; A.tu = tu; A.n_rows = n_rows;
  A.coords = coords; A.cphi = cphi; A.d_min = d_min;
  A.out = out; A.k = k; A.ex_off = ex_off; A.ex = ex; A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  // candidates per workgroup: "geoie_score_span", or - so that a call of one history still fills the chip - about 4 workgroups per CU
  // over the call, at least 256 candidates each
  int64_t span = c->geo_span;
  if (span <= 0) {
    const int64_t want = ((int64_t)4 * c->num_cu + n_rows - 1) / n_rows;
    span = ((int64_t)P->n_item + want - 1) / want;
    if (span < 256) span = 256;
  }
  span = (span + 15) & ~(int64_t)15;
  if (span > (int64_t)1 << 30) span = (int64_t)1 << 30;
  A.span = (int)span;
  A.n_split = (int)(((int64_t)P->n_item + span - 1) / span);
  if ((int64_t)n_rows * A.n_split >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "%s: n_rows x spans per row must stay below 2^31", who);
  if (k > 0 && A.n_split > 1) {
    const size_t lists = (size_t)n_rows * A.n_split;
    if ((rc = ensure(c, c->geo_ws, lists * (GEO_K_MAX * (sizeof(float) + sizeof(int)) + sizeof(int)), st))) return rc;
    A.part_s = (float*)c->geo_ws.p;
    A.part_i = (int*)(A.part_s + lists * GEO_K_MAX);
    A.part_cnt = A.part_i + lists * GEO_K_MAX;
  }
  c->plan.valid = 1; c->plan.geoie_score_span = A.span; c->plan.geoie_score_splits = A.n_split;
  HIPCHK(c, poi::launch_geoie_score(A, st, &c->tm));
  return POI_OK;
}

int poi_geoie_score_all_geo(poi_ctx* c, const poi_geoie_params* P, const int32_t* off, const int32_t* p, const int32_t* mult, const float* tu,
                            const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min, float* out,
                            void* stream) {
  if (c && n_rows > 0 && !out) return fail(c, POI_EINVAL, "poi_geoie_score_all_geo: NULL out");
  return geoie_score_common(c, "poi_geoie_score_all_geo", P, off, p, mult, tu, rows, n_rows, coords, cphi, d_min, out, nullptr, nullptr, 0, nullptr,
                            nullptr, nullptr, stream);
}

int poi_geoie_score_topk_geo(poi_ctx* c, const poi_geoie_params* P, const int32_t* off, const int32_t* p, const int32_t* mult, const float* tu,
                             const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min, const int32_t* ex_off,
                             const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (k <= 0 || k > GEO_K_MAX) return fail(c, POI_ENOTSUP, "poi_geoie_score_topk_geo supports 1 <= k <= %d (got %d)", GEO_K_MAX, k);
  if (c && n_rows > 0 && !idx_out) return fail(c, POI_EINVAL, "poi_geoie_score_topk_geo: NULL idx_out");
  return geoie_score_common(c, "poi_geoie_score_topk_geo", P, off, p, mult, tu, rows, n_rows, coords, cphi, d_min, nullptr, ex_off, ex, k, idx_out,
                            score_out, count_out, stream);
}

// ---------------------------------------------------------------------------------------------
// mini-batch Lstm / Rnn (cells.hip)
static int cell_check(poi_ctx* c, const poi_cell_params* P, const poi_seq_tables* T, bool need_q, const char* who) {
  if (!c || !P || !T) return fail(c, POI_EINVAL, "%s: NULL ctx/params/tables", who);
  if (P->cell != POI_CELL_RNN && P->cell != POI_CELL_LSTM) return fail(c, POI_EINVAL, "%s: cell must be POI_CELL_RNN or POI_CELL_LSTM (got %d)", who, P->cell);
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, P->dim);
  if (!P->lt || !P->ui || !P->wh || !P->bi) return fail(c, POI_EINVAL, "%s: lt/ui/wh/bi must be non-NULL", who);
  if (is_f16(c, P->lt)) return fail(c, POI_ENOTSUP, "%s: float32 tables only", who);
  if (P->n_item <= 0 || (int64_t)P->n_item + 2 >= ((int64_t)1 << 31)) return fail(c, POI_EINVAL, "%s: bad n_item", who);
  if (!T->off || !T->p || (need_q && !T->q)) return fail(c, POI_EINVAL, "%s: tables off/p/q must be non-NULL", who);
  if (T->n_user <= 0 || T->max_len <= 0 || T->len_max < T->max_len) return fail(c, POI_EINVAL, "%s: tables need n_user > 0 and 0 < max_len <= len_max", who);
  return POI_OK;
}

static void cell_fill(poi::CellArgs& A, const poi_cell_params* P, const poi_seq_tables* T, const int32_t* uidx, int n) {
  memset(&A, 0, sizeof A);
  A.lt = P->lt; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.n_item = P->n_item; A.dim = P->dim; A.G = P->cell;
  A.off = T->off; A.p = T->p; A.q = T->q; A.n_user = T->n_user; A.len_max = T->len_max; A.max_len = T->max_len;
  A.uidx = uidx; A.n_seq = n;
}

int poi_cell_step(poi_ctx* c, const poi_cell_params* P, const poi_seq_tables* T, const int32_t* uidx, int32_t n, float alpha, float lambda,
                  float* out, void* stream) {
  int rc = cell_check(c, P, T, true, "poi_cell_step");
  if (rc) return rc;
  if (!uidx || !out || n < 0) return fail(c, POI_EINVAL, "poi_cell_step: uidx/out NULL or n < 0");
  if (n == 0) return POI_OK;
  const size_t R = (size_t)n * (size_t)T->max_len, E = 2 * R + 1;
  if (E >= ((size_t)1 << 31) - 128) return fail(c, POI_ENOTSUP, "poi_cell_step: n_seq x max_len must stay below 2^30");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.tick();
  poi::CellArgs A;
  cell_fill(A, P, T, uidx, n);
  A.out = out; A.alpha = shortest_decimal(alpha); A.lambda = shortest_decimal(lambda);
  A.grid = poi::cell_grid(n, c->cell_grid); A.ch_rows = poi::cell_chunk_rows(n, T->max_len);
  c->plan = poi_ctx::LastPlan{}; c->plan.valid = 1; c->plan.cell_kernel = P->cell; c->plan.cell_grid = A.grid;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const size_t D = (size_t)P->dim, NO = (size_t)P->cell * D, Rp = R + 8, Ep = E + 64, chunks = (E + 63) / 64 + 2;
  const size_t n_f4 = 4 * NO * (D / 4) + chunks;                                         // packed weights, meta
  const size_t n_dbl = Rp * (3 * D + NO + 1) + (size_t)CELL_DENSE_CHUNKS * NO * (2 * D + 1) + 2 * chunks * D;
  const size_t n_i32 = Ep * D + 4 * Ep + Rp + 2 * ((size_t)n + 8) + 64 + chunks + RS_HIST_INTS + RS_MAXBIN;
  if ((rc = ensure(c, c->cell_ws, 16 * n_f4 + 8 * n_dbl + 4 * n_i32 + 256, st))) return rc;
  float4* f4 = (float4*)c->cell_ws.p;
  A.uiP = f4; f4 += NO * (D / 4); A.whP = f4; f4 += NO * (D / 4); A.uiT = f4; f4 += NO * (D / 4); A.whT = f4; f4 += NO * (D / 4);
  A.meta = (int4*)f4; f4 += chunks;
  double* dp = (double*)f4;
  A.H = dp; dp += Rp * D; A.ACT = dp; dp += Rp * NO; A.CS = dp; dp += Rp * D; A.DX = dp; dp += Rp * D; A.gam = dp; dp += Rp;
  A.dpart = dp; dp += (size_t)CELL_DENSE_CHUNKS * NO * (2 * D + 1);
  A.lead = dp; dp += chunks * D; A.trail = dp; dp += chunks * D;
  A.slot = (float*)dp;
  int* ip = (int*)(A.slot + Ep * D);
  A.keys0 = ip; ip += Ep; A.keys1 = ip; ip += Ep; A.vals0 = ip; ip += Ep; A.vals1 = ip; ip += Ep;
  A.rowp = ip; ip += Rp; A.slen = ip; ip += n + 8; A.poff = ip; ip += n + 8; A.cnt = ip; ip += 64; A.mm = ip; ip += chunks;
  A.hist = ip;
  HIPCHK(c, poi::launch_cell_step(A, st, &c->tm));
  return POI_OK;
}

int poi_cell_predict(poi_ctx* c, const poi_cell_params* P, const poi_seq_tables* T, const int32_t* uidx, const int32_t* out_row, int32_t n,
                     float* hts, void* stream) {
  int rc = cell_check(c, P, T, false, "poi_cell_predict");
  if (rc) return rc;
  if (!uidx || !hts || n < 0) return fail(c, POI_EINVAL, "poi_cell_predict: uidx/hts NULL or n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::CellArgs A;
  cell_fill(A, P, T, uidx, n);
  A.out_row = out_row; A.hts = hts; A.grid = poi::cell_grid(n, c->cell_grid);
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const size_t D = (size_t)P->dim, NO = (size_t)P->cell * D;
  if ((rc = ensure(c, c->cell_ws, 16 * 4 * NO * (D / 4) + 256, st))) return rc;
  float4* f4 = (float4*)c->cell_ws.p;
  A.uiP = f4; f4 += NO * (D / 4); A.whP = f4; f4 += NO * (D / 4); A.uiT = f4; f4 += NO * (D / 4); A.whT = f4;
  HIPCHK(c, poi::launch_cell_predict(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// online sessions (session.hip)
// ---------------------------------------------------------------------------------------------
static int session_check(poi_ctx* c, const poi_gru_params* P, bool spatial, const char* who) {
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, P->dim);
  if (P->n_item <= 0) return fail(c, POI_EINVAL, "%s: n_item must be positive", who);
  if (spatial && (!P->di || !P->vs || !P->bs || P->n_dist <= 0)) return fail(c, POI_EINVAL, "%s: the spatial cell needs di / vs / bs and n_dist > 0", who);
  if (!spatial && (P->di || P->vs || P->bs || P->n_dist != 0)) return fail(c, POI_EINVAL, "%s: the plain cell takes di / vs / bs NULL and n_dist 0", who);
  if (spatial && P->n_dist + 1 > 4096) return fail(c, POI_ENOTSUP, "%s: at most 4095 distance bins", who);
  if (spatial && is_f16(c, P->di)) return fail(c, POI_ENOTSUP, "%s: the distance table must be float32 (only the POI snapshot may be a half table)", who);
  return POI_OK;
}

static void session_fill(poi_ctx* c, poi::SessArgs& A, const poi_gru_params* P, bool spatial) {
  A = poi::SessArgs{};
  A.lt = P->lt; A.lt_f16 = is_f16(c, P->lt);
  A.di = P->di; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.vs = P->vs; A.bs = P->bs;
  A.n_item = P->n_item; A.n_dist = spatial ? P->n_dist : 0; A.dim = P->dim; A.xw = spatial ? 2 * P->dim : P->dim; A.spatial = spatial ? 1 : 0;
}

int poi_session_advance(poi_ctx* c, const poi_gru_params* P, const double* coords, const double* cphi, const double* thr, double dd,
                        double* h, float* sts, int32_t* last_poi, int32_t* steps, int32_t n_slot, const int32_t* slot,
                        const int32_t* poi, int32_t n, float* hts_out, float* sts_out, void* stream) {
  if (!c || !P) return fail(c, POI_EINVAL, "poi_session_advance: NULL ctx/params");
  if (!P->lt || !P->ui || !P->wh || !P->bi) return fail(c, POI_EINVAL, "poi_session_advance: lt/ui/wh/bi must be non-NULL");
  const bool spatial = P->di != nullptr || P->n_dist != 0;
  int rc = session_check(c, P, spatial, "poi_session_advance");
  if (rc) return rc;
  if (spatial && (!coords || !cphi || !thr || !sts || !(dd > 0))) return fail(c, POI_EINVAL, "poi_session_advance: the spatial cell needs coords / cphi / thr / sts and dd > 0");
  if (!h || !last_poi || !steps || n_slot <= 0) return fail(c, POI_EINVAL, "poi_session_advance: h / last_poi / steps NULL or n_slot <= 0");
  if (!slot || !poi || n < 0) return fail(c, POI_EINVAL, "poi_session_advance: slot / poi NULL or n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::SessArgs A;
  session_fill(c, A, P, spatial);
  A.coords = coords; A.cphi = cphi; A.thr = thr; A.dd = dd;
  A.h = h; A.sts = sts; A.last_poi = last_poi; A.steps = steps; A.n_slot = n_slot;
  A.slot = slot; A.poi = poi; A.n = n; A.hts_out = hts_out; A.sts_out = sts_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const int tile = n >= c->sess_tile_min && poi::sess_tile_supported(A.dim, A.xw, A.n_dist + 1, A.spatial);
  // repeated slots: one event needs no check, small event launches scan the call inside the kernel, everything else claims the slots
  if (n > 1 && (tile || n > SESS_SCAN_MAX)) {
    if ((rc = ensure(c, c->sess_owner, sizeof(int) * (size_t)n_slot, st))) return rc;
    A.owner = (int*)c->sess_owner.p;
  }
  c->plan.valid = 1; c->plan.session_path = tile; c->plan.session_tiles = tile ? (n + 15) / 16 : 0; c->plan.session_tile_min = c->sess_tile_min;
  HIPCHK(c, poi::launch_session(A, tile, st, &c->tm));
  return POI_OK;
}

int poi_session_sts(poi_ctx* c, const poi_gru_params* P, const double* h, int32_t n_slot, const int32_t* slot, int32_t n, float* sts_out,
                    void* stream) {
  if (!c || !P) return fail(c, POI_EINVAL, "poi_session_sts: NULL ctx/params");
  int rc = session_check(c, P, true, "poi_session_sts");
  if (rc) return rc;
  if (!h || !slot || !sts_out || n < 0 || n_slot <= 0) return fail(c, POI_EINVAL, "poi_session_sts: h / slot / sts_out NULL, n < 0 or n_slot <= 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::SessArgs A;
  session_fill(c, A, P, true);
  A.h = const_cast<double*>(h); A.n_slot = n_slot; A.slot = slot; A.n = n; A.sts_out = sts_out; A.head_only = 1;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  HIPCHK(c, poi::launch_session(A, 0, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// online sessions of Lstm / Rnn / CA-RNN (session_cells.hip)
// ---------------------------------------------------------------------------------------------
static int session_cells_run(poi_ctx* c, poi::SessCellArgs& A, const char* who, void* stream) {
  if (A.dim <= 0 || A.dim % 4 != 0 || A.dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, A.dim);
  if (is_f16(c, A.lt)) return fail(c, POI_ENOTSUP, "%s: float32 tables only", who);
  if (A.n_item <= 0) return fail(c, POI_EINVAL, "%s: n_item must be positive", who);
  if (!A.h || !A.last_poi || !A.steps || A.n_slot <= 0) return fail(c, POI_EINVAL, "%s: h / last_poi / steps NULL or n_slot <= 0", who);
  if (!A.slot || !A.poi || A.n < 0) return fail(c, POI_EINVAL, "%s: slot / poi NULL or n < 0", who);
  if (A.n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const int tile = A.n >= c->sess_tile_min && poi::sess_cell_tile_supported(A.G, A.dim);
  // repeated slots: as poi_session_advance - one event needs no check, small event launches scan the call inside the kernel
  if (A.n > 1 && (tile || A.n > SESS_SCAN_MAX)) {
    if ((rc = ensure(c, c->sess_owner, sizeof(int) * (size_t)A.n_slot, st))) return rc;
    A.owner = (int*)c->sess_owner.p;
  }
  if (tile && A.G == 0) {
    if ((rc = ensure(c, c->sess_wrs, sizeof(double) * (size_t)(A.n_dist + 1) * A.dim, st))) return rc;
    A.wrs = (const double*)c->sess_wrs.p;
  }
  c->plan.valid = 1; c->plan.session_path = tile; c->plan.session_tiles = tile ? (A.n + 15) / 16 : 0; c->plan.session_tile_min = c->sess_tile_min;
  HIPCHK(c, poi::launch_session_cells(A, tile, st, &c->tm));
  return POI_OK;
}

int poi_session_cell_advance(poi_ctx* c, const poi_cell_params* P, double* h, double* cst, int32_t* last_poi, int32_t* steps, int32_t n_slot,
                             const int32_t* slot, const int32_t* poi, int32_t n, float* hts_out, void* stream) {
  if (!c || !P) return fail(c, POI_EINVAL, "poi_session_cell_advance: NULL ctx/params");
  if (P->cell != POI_CELL_RNN && P->cell != POI_CELL_LSTM) return fail(c, POI_EINVAL, "poi_session_cell_advance: cell must be POI_CELL_RNN or POI_CELL_LSTM (got %d)", P->cell);
  if (!P->lt || !P->ui || !P->wh || !P->bi) return fail(c, POI_EINVAL, "poi_session_cell_advance: lt/ui/wh/bi must be non-NULL");
  if (P->cell == POI_CELL_LSTM && !cst) return fail(c, POI_EINVAL, "poi_session_cell_advance: the Lstm cell needs c");
  poi::SessCellArgs A = poi::SessCellArgs{};
  A.G = P->cell; A.lt = P->lt; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.n_item = P->n_item; A.dim = P->dim;
  A.h = h; A.c = P->cell == POI_CELL_LSTM ? cst : nullptr; A.last_poi = last_poi; A.steps = steps; A.n_slot = n_slot;
  A.slot = slot; A.poi = poi; A.n = n; A.hts_out = hts_out;
  return session_cells_run(c, A, "poi_session_cell_advance", stream);
}

int poi_session_carnn_advance(poi_ctx* c, const poi_carnn_params* P, const double* coords, const double* cphi, const double* thr, double dd,
                              double* h, int32_t* last_poi, int32_t* steps, int32_t n_slot, const int32_t* slot, const int32_t* poi, int32_t n,
                              float* hts_out, void* stream) {
  if (!c || !P) return fail(c, POI_EINVAL, "poi_session_carnn_advance: NULL ctx/params");
  if (!P->lt || !P->wd || !P->M || P->n_dist <= 0) return fail(c, POI_EINVAL, "poi_session_carnn_advance: CA-RNN needs lt / wd / M and n_dist > 0");
  if (!coords || !cphi || !thr || !(dd > 0)) return fail(c, POI_EINVAL, "poi_session_carnn_advance: coords / cphi / thr NULL or dd <= 0");
  poi::SessCellArgs A = poi::SessCellArgs{};
  A.G = 0; A.lt = P->lt; A.ui = P->M; A.wh = P->wd; A.n_item = P->n_item; A.n_dist = P->n_dist; A.dim = P->dim;
  A.coords = coords; A.cphi = cphi; A.thr = thr; A.dd = dd;
  A.h = h; A.last_poi = last_poi; A.steps = steps; A.n_slot = n_slot;
  A.slot = slot; A.poi = poi; A.n = n; A.hts_out = hts_out;
  return session_cells_run(c, A, "poi_session_carnn_advance", stream);
}

// ---------------------------------------------------------------------------------------------
// POI2Vec (poi2vec.hip)
static int poi2vec_check(poi_ctx* c, const poi_poi2vec_params* P, const char* who) {
  if (!c || !P || !P->xu || !P->wl || !P->pb || !P->routes || !P->lrs || !P->probs || !P->rid) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->xu) || is_f16(c, P->wl) || is_f16(c, P->pb)) return fail(c, POI_ENOTSUP, "POI2Vec tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "POI2Vec: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->depth < 1 || P->depth > 31) return fail(c, POI_ENOTSUP, "POI2Vec: depth must lie in [1, 31] (got %d)", P->depth);
  if (P->n_user <= 0 || P->n_item <= 0 || (int64_t)P->n_node != ((int64_t)1 << P->depth) - 1)
    return fail(c, POI_EINVAL, "%s: bad sizes (n_node must be 2^depth - 1)", who);
  return POI_OK;
}

struct Carver {
  char* base; size_t used = 0;
  explicit Carver(void* p) : base((char*)p) {}
  void* bytes(size_t b) { void* r = base ? (void*)(base + used) : nullptr; used += (b + 255) & ~(size_t)255; return r; }
};

static void poi2vec_carve(poi::P2vArgs& A, Carver& W, int n_slot) {
  const size_t n = (size_t)A.n, P = (size_t)A.n_pos, R = 4 * (size_t)A.depth, D = (size_t)A.dim, E = P * R + 64, T = P + (size_t)A.n_ctx + 64;
  A.ubad = (int*)W.bytes(sizeof(int) * (n + 1)); A.acc = (int*)W.bytes(sizeof(int) * (n + 1)); A.lpos = (int*)W.bytes(sizeof(int) * (n + 1)); A.lctx = (int*)W.bytes(sizeof(int) * (n + 1));
  A.tot = (int*)W.bytes(sizeof(int) * (8)); A.cnt = (int*)W.bytes(sizeof(int) * (8));
  A.pmax = (float*)W.bytes(sizeof(float) * (n * A.n_tile + 1)); A.psum = (double*)W.bytes(sizeof(double) * (n * A.n_tile + 1));
  A.posval = (double*)W.bytes(sizeof(double) * (P + 1)); A.gz = (double*)W.bytes(sizeof(double) * (P * R + 1)); A.cbuf = (double*)W.bytes(sizeof(double) * (P * D + 1)); A.gcbuf = (double*)W.bytes(sizeof(double) * (P * D + 1));
  A.lse = (double*)W.bytes(sizeof(double) * (n + 1)); A.tsum = (double*)W.bytes(sizeof(double) * (n * D + 1)); A.scale = (float*)W.bytes(sizeof(float) * (8)); A.dxu = (float*)W.bytes(sizeof(float) * ((size_t)n_slot * n * D + 1));
  A.keys0 = (int*)W.bytes(sizeof(int) * (E)); A.keys1 = (int*)W.bytes(sizeof(int) * (E)); A.vals0 = (int*)W.bytes(sizeof(int) * (E)); A.vals1 = (int*)W.bytes(sizeof(int) * (E));
  A.k2a = (int*)W.bytes(sizeof(int) * (T)); A.k2b = (int*)W.bytes(sizeof(int) * (T)); A.v2a = (int*)W.bytes(sizeof(int) * (T)); A.v2b = (int*)W.bytes(sizeof(int) * (T)); A.epos = (int*)W.bytes(sizeof(int) * (T));
  A.hist = (int*)W.bytes(sizeof(int) * ((size_t)RS_HIST_INTS + RS_MAXBIN + 64));
}

int poi_poi2vec_step(poi_ctx* c, const poi_poi2vec_params* P, const int32_t* off, const int32_t* tgt, const int32_t* coff, const int32_t* cidx,
                     const int32_t* users, int32_t n, int64_t n_pos, int64_t n_ctx, int32_t len_max, float alpha, float lambda, float* loss_out,
                     void* stream) {
  int rc = poi2vec_check(c, P, "poi_poi2vec_step");
  if (rc) return rc;
  if (!off || !tgt || !coff || !cidx || !users || !loss_out) return fail(c, POI_EINVAL, "poi_poi2vec_step: NULL argument");
  if (n < 0 || n_pos < 0 || n_ctx < 0 || len_max < 0) return fail(c, POI_EINVAL, "poi_poi2vec_step: bad sizes");
  if (n > 4096) return fail(c, POI_ENOTSUP, "POI2Vec: at most 4096 users per launch (got %d)", n);
  if (n_pos * 4 * P->depth >= ((int64_t)1 << 31) - 64 || n_pos + n_ctx >= ((int64_t)1 << 31) - 64)
    return fail(c, POI_ENOTSUP, "POI2Vec: a launch's route occurrences (4 depth per position) and context entries must stay below 2^31");
  if (c->batch_cap == 0.0f) return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::P2vArgs A;
  memset(&A, 0, sizeof A);
  A.xu = P->xu; A.wl = P->wl; A.pb = P->pb; A.routes = P->routes; A.lrs = (const signed char*)P->lrs; A.probs = P->probs; A.rid = P->rid;
  A.n_user = P->n_user; A.n_item = P->n_item; A.n_node = P->n_node; A.depth = P->depth; A.dim = P->dim;
  A.off = off; A.tgt = tgt; A.coff = coff; A.cidx = cidx; A.users = users;
  A.n = n; A.n_pos = (int)n_pos; A.n_ctx = (int)n_ctx; A.len_max = len_max; A.n_tile = (P->n_item + 63) / 64;
  A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.loss = loss_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const int n_slot = A.n_tile < 256 ? A.n_tile : 256;
  Carver dry(nullptr);
  poi2vec_carve(A, dry, n_slot);
  if ((rc = ensure(c, c->pv_ws, dry.used + 256, st))) return rc;
  Carver W(c->pv_ws.p);
  poi2vec_carve(A, W, n_slot);
  HIPCHK(c, poi::launch_poi2vec_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

static int poi2vec_score_common(poi_ctx* c, const poi_poi2vec_params* P, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch,
                                int32_t length, const int32_t* coff, const int32_t* cidx, int32_t axis, int32_t k, float* out, int32_t* idx_out,
                                float* score_out, void* stream, const char* who, const int32_t* ex_off = nullptr, const int32_t* ex = nullptr,
                                int32_t* count_out = nullptr) {
  int rc = poi2vec_check(c, P, who);
  if (rc) return rc;
  if (!leaf_nodes || !users || !coff || !cidx) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (n_batch < 0 || length < 0 || (axis != 0 && axis != 1)) return fail(c, POI_EINVAL, "%s: bad sizes or softmax_axis", who);
  if ((int64_t)n_batch * length >= ((int64_t)1 << 31) / 4) return fail(c, POI_ENOTSUP, "%s: too many rows", who);
  if (n_batch == 0 || length == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::P2vScoreArgs A;
  memset(&A, 0, sizeof A);
  A.xu = P->xu; A.wl = P->wl; A.pb = P->pb; A.probs = P->probs; A.rid = P->rid; A.leaf_nodes = leaf_nodes; A.users = users; A.coff = coff; A.cidx = cidx;
  A.n_user = P->n_user; A.n_item = P->n_item; A.n_node = P->n_node; A.depth = P->depth; A.dim = P->dim;
  A.n_batch = n_batch; A.length = length; A.n_rows = n_batch * length; A.axis = axis; A.k = k;
  const size_t rows = (size_t)A.n_rows, NL = (size_t)1 << (P->depth - 1);
  for (int pass = 0; pass < 2; ++pass) {
    Carver W(pass ? c->pv_sc.p : nullptr);
    A.cl = (double*)W.bytes(sizeof(double) * (rows * P->dim)); A.zf = (double*)W.bytes(sizeof(double) * (rows * P->n_node)); A.rp = (double*)W.bytes(sizeof(double) * (rows * NL));
    const size_t ns = (size_t)(axis == 0 ? P->n_item : n_batch);
    A.ssum = (double*)W.bytes(sizeof(double) * (ns)); A.smax = (float*)W.bytes(sizeof(float) * (ns)); A.logit = (float*)W.bytes(sizeof(float) * ((size_t)n_batch * P->n_item));
    A.out = out;                                     // NULL for the top-K: the scores are not stored
    if (!pass && (rc = ensure(c, c->pv_sc, W.used + 256, st))) return rc;
  }
  A.idx_out = idx_out; A.score_out = score_out;
  A.ex_off = ex_off; A.ex = ex; A.count_out = count_out;
  HIPCHK(c, poi::launch_poi2vec_scores(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

int poi_poi2vec_scores(poi_ctx* c, const poi_poi2vec_params* P, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch, int32_t length,
                       const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, float* out, void* stream) {
  if (c && !out) return fail(c, POI_EINVAL, "poi_poi2vec_scores: NULL argument");
  return poi2vec_score_common(c, P, leaf_nodes, users, n_batch, length, coff, cidx, softmax_axis, 0, out, nullptr, nullptr, stream, "poi_poi2vec_scores");
}

int poi_poi2vec_topk(poi_ctx* c, const poi_poi2vec_params* P, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch, int32_t length,
                     const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, int32_t k, int32_t* idx_out, float* score_out, void* stream) {
  if (c && !idx_out) return fail(c, POI_EINVAL, "poi_poi2vec_topk: NULL argument");
  if (c && P && (k < 1 || k > 64 || k > P->n_item)) return fail(c, POI_EINVAL, "poi_poi2vec_topk: k must lie in [1, min(64, n_item)]");
  return poi2vec_score_common(c, P, leaf_nodes, users, n_batch, length, coff, cidx, softmax_axis, k, nullptr, idx_out, score_out, stream, "poi_poi2vec_topk");
}

int poi_poi2vec_topk_ex(poi_ctx* c, const poi_poi2vec_params* P, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch, int32_t length,
                        const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, const int32_t* ex_off, const int32_t* ex, int32_t k,
                        int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (c && !idx_out) return fail(c, POI_EINVAL, "poi_poi2vec_topk_ex: NULL argument");
  if (c && ((ex_off == nullptr) != (ex == nullptr))) return fail(c, POI_EINVAL, "poi_poi2vec_topk_ex: ex_off and ex come together");
  if (c && P && (k < 1 || k > 64 || k > P->n_item)) return fail(c, POI_EINVAL, "poi_poi2vec_topk_ex: k must lie in [1, min(64, n_item)]");
  return poi2vec_score_common(c, P, leaf_nodes, users, n_batch, length, coff, cidx, softmax_axis, k, nullptr, idx_out, score_out, stream,
                              "poi_poi2vec_topk_ex", ex_off, ex, count_out);
}

// fold-in of new users for POI2Vec (foldin_p2v.hip).  The partials grow with users x spans x (dim + 2): the call is cut into user
// chunks that keep them within P2V_FOLD_PART_BYTES (a user's bits do not depend on the chunking)
#define P2V_FOLD_PART_BYTES ((size_t)64 << 20)
int poi_foldin_p2v_span(void) { return P2V_FOLD_SPAN; }

int poi_foldin_p2v(poi_ctx* c, const float* wl, int32_t n_item, int32_t dim, const int32_t* off, const int32_t* tgt, int32_t n, int32_t epochs,
                   float alpha, float lambda, const float* w0, float* w_out, float* loss_out, void* stream) {
  if (!c || !wl || !w_out) return fail(c, POI_EINVAL, "poi_foldin_p2v: NULL ctx / wl / w_out");
  if (dim <= 0 || dim % 4 != 0 || dim > 128) return fail(c, POI_ENOTSUP, "poi_foldin_p2v: dim must be a multiple of 4 in [4, 128] (got %d)", dim);
  if (n < 0 || n_item <= 0 || epochs < 0) return fail(c, POI_EINVAL, "poi_foldin_p2v: n < 0, n_item <= 0 or epochs < 0");
  if (n == 0) return POI_OK;
  if (!off || !tgt) return fail(c, POI_EINVAL, "poi_foldin_p2v: NULL off / tgt");
  if (is_f16(c, wl) || (w0 && is_f16(c, w0)) || is_f16(c, w_out)) return fail(c, POI_ENOTSUP, "poi_foldin_p2v: wl / w0 / w_out must be float32");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  const int n_span = (n_item + P2V_FOLD_SPAN - 1) / P2V_FOLD_SPAN;
  const size_t per_user = sizeof(double) * (size_t)n_span * (size_t)(dim + 2);
  size_t uc = P2V_FOLD_PART_BYTES / per_user / P2V_FOLD_USERS * P2V_FOLD_USERS;
  if (uc < P2V_FOLD_USERS) uc = P2V_FOLD_USERS;
  if (uc > (size_t)n) uc = (size_t)n;
  for (int pass = 0; pass < 2; ++pass) {
    Carver W(pass ? c->pv_fold.p : nullptr);
    double* w = (double*)W.bytes(sizeof(double) * uc * dim);
    double* tbar = (double*)W.bytes(sizeof(double) * uc * dim);
    int* flag = (int*)W.bytes(sizeof(int) * uc);
    double* part = (double*)W.bytes(per_user * uc);
    if (!pass) { if ((rc = ensure(c, c->pv_fold, W.used + 256, st))) return rc; continue; }
    for (size_t r0 = 0; r0 < (size_t)n; r0 += uc) {
      poi::FoldP2vArgs A = {};
      A.wl = wl; A.n_item = n_item; A.dim = dim; A.epochs = epochs; A.n_span = n_span;
      A.n = (int)((size_t)n - r0 < uc ? (size_t)n - r0 : uc);
      A.off = off + r0; A.tgt = tgt; A.alpha = alpha; A.lambda = lambda;
      A.w0 = w0 ? w0 + r0 * dim : nullptr; A.w_out = w_out + r0 * dim; A.loss_out = loss_out ? loss_out + r0 * epochs : nullptr;
      A.w = w; A.tbar = tbar; A.flag = flag; A.part = part; A.bad = (int*)c->bad_ids.p;
      HIPCHK(c, poi::launch_foldin_p2v(A, st, &c->tm));
    }
  }
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
struct UlptaiArg { const void* bins; int bin_bytes; const float* sts; int n_dist; const double *coords, *cphi, *thr; const int* last_poi; double dd; };

static int score_common(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                        const float* wd, const float* prob, float* scores, int32_t k, int32_t* idx_out, float* score_out,
                        void* stream, const UlptaiArg* U = nullptr) {
  // the top-K seed is "consumed by the next call" whatever that call does: taken (and cleared) before any early return, so a failed or
  // empty call can never leave a stale pointer - sized for another n - armed for a later one
  const int32_t* seed_idx = c ? c->seed_idx : nullptr; const int seed_k = c ? c->seed_k : 0;
  if (c) { c->seed_idx = nullptr; c->seed_k = 0; }
  if (!c || !users || !items) return fail(c, POI_EINVAL, "score: NULL argument");
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "bad sizes");
  if (prob && !wd) return fail(c, POI_EINVAL, "prob given without wd");
  if (k < 0 || k > 32 || (k > 0 && k > n_item)) return fail(c, POI_ENOTSUP, "top-K supports 1 <= k <= min(32, n_item) (got %d)", k);
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::ScoreArgs A;
  memset(&A, 0, sizeof A);
  A.users = users; A.items = items; A.items_f16 = is_f16(c, items); A.n = n; A.n_item = n_item; A.dim = dim; A.wd = wd; A.prob = prob;
  A.scores = scores; A.k = k; A.idx_out = idx_out; A.score_out = score_out;
  if (U) { A.ulptai = U->bins; A.bin_bytes = U->bin_bytes; A.sts = U->sts; A.n_dist = U->n_dist; }
  if (U && !U->bins) { A.geo = 1; A.coords = U->coords; A.cphi = U->cphi; A.thr = U->thr; A.last_poi = U->last_poi; A.dd = U->dd; }
  if (const char* e = getenv("POI_SCORE_DBG")) A.dbg = atoi(e);
  const int ntile = (n_item + 31) / 32;
  // variant: 0 = one item stream per wave (row-per-lane loads; small n or dim > 128), 1 = packed item
  // stream per wave with the user tile's A fragments in LDS (default for n >= 128)
  int variant = (n >= 128 && dim <= 128) ? 1 : 0;
  if (c->score_variant >= 0 && dim <= 128) variant = c->score_variant;
  if (U && U->bins) variant = 1;      // the bin matrix is laid out for the packed-stream kernel
  if (U && !U->bins) variant = 0;     // bins on the fly: the row-per-lane kernel (any dim <= 256)
  // ... or, for enough users to fill the chip with eight-wave workgroups and a wide model, the packed-stream GEO kernel
  if (U && !U->bins && k > 0 && n >= 1024 && dim >= 128 && poi::score_geo_stream_lds(dim, U->n_dist) <= 160 * 1024 && c->score_variant != 0) variant = 2;
  const int n_utile = (n + 31) / 32;
  // item ranges per user tile for a table of nt item tiles: long item streams keep per-user thresholds high (few top-K compactions)
  auto splits_for = [&](int nt) {
    int want = (c->num_cu * 8 + n_utile - 1) / n_utile;   // 8 waves per CU
    if (want > nt / 8) want = nt / 8;          // >= 8 tiles per stream: amortise the per-wave top-K epilogue
    if (want < 1) want = 1;
    if (want < (nt + 2046) / 2047) want = (nt + 2046) / 2047;      // candidate lists hold 16-bit item offsets: < 65536 items per range
    return variant == 2 ? ((want + 7) / 8) * 8 : ((want + 3) / 4) * 4;
  };
  const int n_split = splits_for(ntile);
  A.n_split = n_split;
  const int n_pad = n_utile * 32;
  int rc;
  // one-stage kernel of the chosen variant + merge of the per-range lists, on the item table X describes
  auto one_stage = [&](poi::ScoreArgs& X) -> int {
    const int nt = (X.n_item + 31) / 32;
    if (variant == 2) {
      const int d8 = dim <= 128 ? 16 : 32;
      int r2 = ensure(c, c->items_pk, sizeof(float) * 4 * (size_t)nt * d8 * 64, st);
      if (r2) return r2;
      X.items_packed = (float4*)c->items_pk.p;
      HIPCHK(c, poi::launch_score_geo_stream(X, st, &c->tm));
    } else if (variant == 1) {
      const int d8 = dim <= 32 ? 4 : dim <= 64 ? 8 : 16;
      int r2 = ensure(c, c->items_pk, sizeof(float) * 4 * (size_t)nt * d8 * 64, st);
      if (r2) return r2;
      X.items_packed = (float4*)c->items_pk.p;
      HIPCHK(c, poi::launch_score_packed(X, st, &c->tm));
    } else {
      HIPCHK(c, poi::launch_score(X, st, &c->tm));
    }
    if (k > 0) HIPCHK(c, poi::launch_topk_merge(X, X.n_split, n_pad, st));
    return POI_OK;
  };
  bool two_stage = false, use_maxpass = false;
  if (k > 0) {
    const size_t cand = (size_t)n_split * n_pad * k;
    if ((rc = ensure(c, c->cand_s, sizeof(float) * cand, st))) return rc;
    if ((rc = ensure(c, c->cand_i, sizeof(int) * cand, st))) return rc;
    A.cand_score = (float*)c->cand_s.p; A.cand_idx = (int*)c->cand_i.p;
    const bool seeded = seed_idx && seed_k >= k && seed_k <= 64;
    {
      poi::ScoreArgs probe = A; probe.seeded = 1;
      two_stage = c->topk_filter && (variant == 1 || A.geo) && poi::score_two_stage_supported(probe);
    }
    // SELF-SEEDING pre-pass of the two-stage path: the one-stage kernel on the first 1/16 of the item tiles (1/64 when the caller's
    // seed already gave bounds) - the K-th best EXACT score of any subset is a lower bound of the final K-th best, so the filter pass
    // starts from thresholds that leave ~16 K (64 K) survivors per user whatever the seed holds: an unseeded call (the first evaluation
    // of a run) or a useless seed (a model that moved a lot) no longer sends its tiles to the one-stage kernel.  Unseeded calls always
    // take it; seeded ones when the table has >= 2^20 items (there it costs < 2 % of the call).
    const int sub_tiles = !two_stage ? 0 : !seeded ? (ntile >= 256 ? ntile / 16 : 0) : (n_item >= (1 << 20) ? ntile / 64 : 0);
    if (two_stage && !seeded && sub_tiles == 0) two_stage = false;      // (a small table and no seed: one-stage)
    if (n_split > 1 || seeded || two_stage) {
      if ((rc = ensure(c, c->gbound, sizeof(unsigned) * (size_t)n_pad, st))) return rc;
      HIPCHK(c, hipMemsetAsync(c->gbound.p, 0, sizeof(unsigned) * (size_t)n_pad, st));
      A.gbound = (unsigned*)c->gbound.p;
    }
    if (seeded) {
      c->tm.begin("topk_seed", st);
      HIPCHK(c, poi::launch_topk_seed(A, seed_idx, seed_k, st));
      c->tm.end(st);
      A.seeded = 1;
    }
    // unseeded, resident bin matrix / no distance term, dims 64 / 128: thresholds from the block maxima of the f16 lower bounds instead
    // (score_filter.hip, MAXP: one f16 pass over ALL items, ~1.3 K survivors per user against ~17 K of the float32 prefix pre-pass)
    use_maxpass = two_stage && !seeded && sub_tiles > 0 && poi::score_maxpass_supported(A);
    if (const char* e = getenv("POI_SF_MAXPASS")) use_maxpass = use_maxpass && atoi(e) != 0;
    if (two_stage && sub_tiles > 0 && !use_maxpass) {
      if ((rc = ensure(c, c->pre_idx, sizeof(int) * (size_t)n_pad * k, st)) || (rc = ensure(c, c->pre_sc, sizeof(float) * (size_t)n_pad * k, st))) return rc;
      poi::ScoreArgs S = A;
      S.n_item = sub_tiles * 32; S.bins_ntile = ntile; S.n_split = splits_for(sub_tiles);
      S.idx_out = (int*)c->pre_idx.p; S.score_out = (float*)c->pre_sc.p;
      if ((size_t)S.n_split * n_pad * k > cand) {
        if ((rc = ensure(c, c->cand_s, sizeof(float) * (size_t)S.n_split * n_pad * k, st)) || (rc = ensure(c, c->cand_i, sizeof(int) * (size_t)S.n_split * n_pad * k, st))) return rc;
        A.cand_score = S.cand_score = (float*)c->cand_s.p; A.cand_idx = S.cand_idx = (int*)c->cand_i.p;
      }
      if ((rc = one_stage(S))) return rc;
      HIPCHK(c, poi::launch_topk_bound(S.score_out, n, k, A.gbound, st));
      A.seeded = 1;
    }
  }
  if (two_stage) {
    // two-stage: f16 filter pass + exact float32 rescoring of the survivors (score_filter.hip); the one-stage kernel below then only
    // runs the user tiles whose survivor lists overflowed (A.tile_flag)
    const int kg = dim / 16, cap = poi::score_filter_cap();
    if ((rc = ensure(c, c->items_pk16, sizeof(uint4) * (size_t)ntile * kg * 64, st)) || (rc = ensure(c, c->inorm, sizeof(float2) * (size_t)ntile * 32, st)) ||
        (rc = ensure(c, c->surv_cnt, sizeof(int) * (size_t)n_pad, st)) || (rc = ensure(c, c->surv_idx, sizeof(int) * (size_t)n_pad * cap, st)) ||
        (rc = ensure(c, c->surv_sc, sizeof(float) * (size_t)n_pad * cap, st)) ||
        (rc = ensure(c, c->tflag, sizeof(int) * (size_t)n_utile, st))) return rc;
    HIPCHK(c, hipMemsetAsync(c->surv_cnt.p, 0, sizeof(int) * (size_t)n_pad, st));
    HIPCHK(c, hipMemsetAsync(c->tflag.p, 0, sizeof(int) * (size_t)n_utile, st));
    A.items_packed16 = (const uint4*)c->items_pk16.p; A.inorm = (const float2*)c->inorm.p;
    A.surv_cnt = (int*)c->surv_cnt.p; A.surv_idx = (int*)c->surv_idx.p; A.surv_sc = (float*)c->surv_sc.p; A.tile_flag = (int*)c->tflag.p;
    // GEO with a huge item table and few users (config X's evaluation): the item-stationary filter - every user tile's own pass over the
    // item table is 1.3 TB at 8192 users x 10 M POIs; forced (2) / forbidden (0) by POI_SF_ITEMS for tests and A/B runs
    A.n_cu = c->num_cu;
    {
      int items_mode = (A.geo && n_item >= (1 << 20) && n_utile <= 4096) ? 1 : 0;
      if (const char* e = getenv("POI_SF_ITEMS")) items_mode = A.geo ? (atoi(e) != 0) : 0;
      if (c->sf_items >= 0) items_mode = A.geo ? c->sf_items : 0;
      if (items_mode) {
        if ((rc = ensure(c, c->users_pk16, sizeof(uint4) * (size_t)n_utile * kg * 64, st)) || (rc = ensure(c, c->ubound, sizeof(float) * 4 * (size_t)n_pad, st)) ||
            (rc = ensure(c, c->ugeo, sizeof(double) * 3 * (size_t)n_pad, st))) return rc;
        A.users_packed16 = (uint4*)c->users_pk16.p; A.ubound = (float4*)c->ubound.p; A.ugeo = (double*)c->ugeo.p;
      }
    }
    int nsf = ((4 * c->num_cu + n_utile - 1) / n_utile) * 4;      // >= 4 workgroups (16 waves) per CU
    if (nsf < 16) nsf = 16;      // (swept at the Gowalla shape: 8 / 16 / 32 / 64 / 128 ranges -> 3.09 / 2.84 / 2.80 / 2.86 / 3.21 ms of filter time)
    if (const char* e = getenv("POI_SF_NSPLIT")) { const int v = atoi(e); if (v >= 4) nsf = (v / 4) * 4; }      // tuning switch
    if (nsf > (ntile / 4) * 4) nsf = (ntile / 4) * 4;
    if (nsf < 4) nsf = 4;
    if (use_maxpass) {
      HIPCHK(c, poi::launch_score_maxpass(A, nsf, st, &c->tm));
      A.seeded = 1;
    }
    HIPCHK(c, poi::launch_score_two_stage(A, nsf, st, &c->tm));
    c->last_two_n = n; c->last_two_tiles = n_utile;
  }
  return one_stage(A);
}

int poi_score_all(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                  const float* wd, const float* prob, float* scores_out, void* stream) {
  if (!scores_out) return fail(c, POI_EINVAL, "scores_out is NULL");
  return score_common(c, users, items, n, n_item, dim, wd, prob, scores_out, 0, nullptr, nullptr, stream);
}

int poi_score_topk(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                   const float* wd, const float* prob, int32_t k, int32_t* idx_out, float* score_out, void* stream) {
  if (!idx_out || k <= 0) return fail(c, POI_EINVAL, "idx_out NULL or k <= 0");
  return score_common(c, users, items, n, n_item, dim, wd, prob, nullptr, k, idx_out, score_out, stream);
}

int poi_ulptai_build(poi_ctx* c, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                     int32_t n_user, int32_t n_item, int32_t n_dist, double dd, void* out, int32_t bin_bytes, void* stream) {
  if (!c || !coords || !cphi || !thr || !last_poi || !out) return fail(c, POI_EINVAL, "poi_ulptai_build: NULL argument");
  if (n_user <= 0 || n_item <= 0 || n_dist <= 0 || !(dd > 0)) return fail(c, POI_EINVAL, "bad sizes");
  if (bin_bytes != 1 && bin_bytes != 2) return fail(c, POI_EINVAL, "bin_bytes must be 1 or 2");
  if ((bin_bytes == 1 && n_dist > 255) || n_dist > 65535) return fail(c, POI_EINVAL, "n_dist %d does not fit %d-byte bins", n_dist, bin_bytes);
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("ulptai_build", (hipStream_t)stream);
  HIPCHK(c, poi::launch_ulptai(coords, cphi, thr, last_poi, n_user, n_item, n_dist, dd, out, bin_bytes, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_score_topk_ulptai(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                          const float* wd, const float* sts, const void* ulptai, int32_t bin_bytes, int32_t n_dist,
                          int32_t k, int32_t* idx_out, float* score_out, void* stream) {
  if (!idx_out || k <= 0) return fail(c, POI_EINVAL, "idx_out NULL or k <= 0");
  if (!wd || !sts || !ulptai) return fail(c, POI_EINVAL, "poi_score_topk_ulptai: wd / sts / ulptai NULL");
  if (bin_bytes != 1 && bin_bytes != 2) return fail(c, POI_EINVAL, "bin_bytes must be 1 or 2");
  if (dim > 128) return fail(c, POI_ENOTSUP, "the bin-matrix path supports dim <= 128 (got %d)", dim);
  if (n_dist <= 0 || (int64_t)n * (n_dist + 1) >= (int64_t)1 << 31) return fail(c, POI_EINVAL, "n * (n_dist + 1) must stay below 2^31: score in batches");
  const UlptaiArg U{ulptai, bin_bytes, sts, n_dist, nullptr, nullptr, nullptr, nullptr, 0.0};
  return score_common(c, users, items, n, n_item, dim, wd, nullptr, nullptr, k, idx_out, score_out, stream, &U);
}

int poi_score_topk_geo(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                       const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                       int32_t k, int32_t* idx_out, float* score_out, void* stream) {
  if (!idx_out || k <= 0) return fail(c, POI_EINVAL, "idx_out NULL or k <= 0");
  if (!wd || !sts || !coords || !cphi || !thr || !last_poi) return fail(c, POI_EINVAL, "poi_score_topk_geo: NULL argument");
  if (n_dist <= 0 || !(dd > 0)) return fail(c, POI_EINVAL, "bad n_dist / dd");
  const UlptaiArg U{nullptr, 0, sts, n_dist, coords, cphi, thr, last_poi, dd};
  return score_common(c, users, items, n, n_item, dim, wd, nullptr, nullptr, k, idx_out, score_out, stream, &U);
}

// ---------------------------------------------------------------------------------------------
// restricted top-K (near.hip)
int poi_score_topk_near(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const double* coords,
                        const double* cphi, const int32_t* lat_order, const int32_t* anchor, double c_r, const int32_t* ex_off, const int32_t* ex,
                        const float* wd, const float* sts, const double* thr, int32_t n_dist, double dd, int32_t k, int32_t* idx_out,
                        float* score_out, int32_t* count_out, void* stream) {
  if (!c || !users || !items || !idx_out) return fail(c, POI_EINVAL, "poi_score_topk_near: NULL ctx / users / items / idx_out");
  if (k <= 0 || k > NEAR_K_MAX) return fail(c, POI_ENOTSUP, "poi_score_topk_near supports 1 <= k <= %d (got %d)", NEAR_K_MAX, k);
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_score_topk_near: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "poi_score_topk_near: n < 0 or n_item <= 0");
  if (!(c_r >= 0.0)) return fail(c, POI_EINVAL, "poi_score_topk_near: c_r must be >= 0 (+inf: no radius test)");
  const bool radius = c_r < HUGE_VAL, geo = wd != nullptr;
  if ((ex_off == nullptr) != (ex == nullptr)) return fail(c, POI_EINVAL, "poi_score_topk_near: ex_off and ex go together");
  if (geo != (sts != nullptr) || geo != (thr != nullptr)) return fail(c, POI_EINVAL, "poi_score_topk_near: wd, sts and thr go together");
  if (geo && (n_dist <= 0 || !(dd > 0))) return fail(c, POI_EINVAL, "poi_score_topk_near: the distance term needs n_dist > 0 and dd > 0");
  if ((radius || geo) && (!coords || !cphi || !anchor)) return fail(c, POI_EINVAL, "poi_score_topk_near: a radius or a distance term needs coords / cphi / anchor");
  if (radius && !lat_order) return fail(c, POI_EINVAL, "poi_score_topk_near: a radius needs lat_order");
  if (is_f16(c, users)) return fail(c, POI_ENOTSUP, "poi_score_topk_near: users must be float32");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::NearArgs A = {};
  A.users = users; A.items = items; A.items_f16 = is_f16(c, items);
  A.n = n; A.n_item = n_item; A.dim = dim; A.k = k;
  A.coords = coords; A.cphi = cphi; A.order = lat_order; A.anchor = anchor; A.c_r = c_r; A.band_deg = radius ? lat_band_deg(c_r) : 0.0;
  A.ex_off = ex_off; A.ex = ex;
  A.wd = wd; A.sts = sts; A.thr = thr; A.n_dist = geo ? n_dist : 0; A.bin_scale = geo ? (float)(12742.0 * 1000.0 / dd) : 0.f;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  // few rows (live traffic): every row's band is cut into slices so that the call fills the CUs; many rows: one workgroup per row
  const int split = n <= c->near_split_max;
  A.n_split = 1;
  if (split) {
    int s = c->near_grid > 0 ? c->near_grid : 4 * c->num_cu / n;
    if (c->near_grid <= 0 && s < 2) s = 2;
    A.n_split = s > NEAR_SPLIT_LIMIT ? NEAR_SPLIT_LIMIT : s;
    const size_t lists = (size_t)n * A.n_split;
    if ((rc = ensure(c, c->near_ws, lists * (NEAR_K_MAX * (sizeof(float) + sizeof(int)) + sizeof(int)), st))) return rc;
    A.part_s = (float*)c->near_ws.p;
    A.part_i = (int*)(A.part_s + lists * NEAR_K_MAX);
    A.part_cnt = A.part_i + lists * NEAR_K_MAX;
  }
  c->plan.valid = 1; c->plan.near_path = split; c->plan.near_splits = split ? A.n_split : 0; c->plan.near_split_max = c->near_split_max;
  HIPCHK(c, poi::launch_near(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// exact target ranks (rank.hip)
static int rank_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* tgt, const int32_t* tmask, int32_t len_t,
                      const int32_t* ex_off, const int32_t* ex, const int32_t* rank_out) {
  if (!tgt || !tmask || !rank_out) return fail(c, POI_EINVAL, "%s: NULL tgt / tmask / rank_out", who);
  if (len_t <= 0 || len_t > RANK_LT_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= len_t <= %d (got %d)", who, RANK_LT_MAX, len_t);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if ((ex_off == nullptr) != (ex == nullptr)) return fail(c, POI_EINVAL, "%s: ex_off and ex go together", who);
  return POI_OK;
}

int poi_score_rank(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                   const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                   const int32_t* tgt, const int32_t* tmask, int32_t len_t, const int32_t* ex_off, const int32_t* ex, int32_t* rank_out,
                   float* score_out, int32_t* count_out, void* stream) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "poi_score_rank: NULL ctx / users / items");
  int rc;
  if ((rc = rank_check(c, "poi_score_rank", n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out))) return rc;
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_score_rank: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  const bool geo = wd != nullptr;
  if (geo && (!sts || !coords || !cphi || !thr || !last_poi)) return fail(c, POI_EINVAL, "poi_score_rank: the distance term needs sts / coords / cphi / thr / last_poi");
  if (geo && (n_dist <= 0 || !(dd > 0))) return fail(c, POI_EINVAL, "poi_score_rank: the distance term needs n_dist > 0 and dd > 0");
  if (is_f16(c, users)) return fail(c, POI_ENOTSUP, "poi_score_rank: users must be float32");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::RankArgs A = {};
  A.users = users; A.items = items; A.items_f16 = is_f16(c, items);
  A.n = n; A.n_item = n_item; A.dim = dim; A.len_t = len_t;
  if (geo) { A.wd = wd; A.sts = sts; A.coords = coords; A.cphi = cphi; A.thr = thr; A.last_poi = last_poi; A.n_dist = n_dist; A.bin_scale = (float)(12742.0 * 1000.0 / dd); }
  A.tgt = tgt; A.tmask = tmask; A.ex_off = ex_off; A.ex = ex;
  A.rank_out = rank_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  const int n_utile = (n + 31) / 32, ntile = (n_item + 31) / 32;
  if ((rc = ensure(c, c->rank_ws, sizeof(poi::RankTgt) * (size_t)n_utile * 32 * RANK_LT_MAX, st))) return rc;
  A.tl = (poi::RankTgt*)c->rank_ws.p;
  // item ranges per 32-row tile, one wave each: 8 waves per CU over the call, at least 8 tiles per range; "rank_grid" caps it; the 16-bit
  // per-lane counters set the floor
  int want = (c->num_cu * 8 + n_utile - 1) / n_utile;
  if (want > ntile / 8) want = ntile / 8;
  if (c->rank_grid > 0 && want > c->rank_grid) want = c->rank_grid;
  if (want < 1) want = 1;
  if (want < (ntile + RANK_TILES_MAX - 1) / RANK_TILES_MAX) want = (ntile + RANK_TILES_MAX - 1) / RANK_TILES_MAX;
  A.n_split = want;
  c->plan.valid = 1; c->plan.rank_splits = want;
  HIPCHK(c, poi::launch_rank(A, st, &c->tm));
  return POI_OK;
}

int poi_rank_scores(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, const int32_t* tgt, const int32_t* tmask, int32_t len_t,
                    const int32_t* ex_off, const int32_t* ex, int32_t* rank_out, int32_t* count_out, void* stream) {
  if (!c || !scores) return fail(c, POI_EINVAL, "poi_rank_scores: NULL ctx / scores");
  int rc;
  if ((rc = rank_check(c, "poi_rank_scores", n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out))) return rc;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  c->tm.begin("rank_scores", st);
  HIPCHK(c, poi::launch_rank_scores(scores, n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out, count_out, (int*)c->bad_ids.p, st));
  c->tm.end(st);
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// group recommendation (group.hip)
static int group_check_args(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* g_off, const int32_t* g_mem, int32_t n_grp,
                            int32_t agg, const int32_t* ex_off, const int32_t* ex, int32_t k, const int32_t* idx_out) {
  if (!g_off || !g_mem || !idx_out) return fail(c, POI_EINVAL, "%s: NULL g_off / g_mem / idx_out", who);
  if (k <= 0 || k > GROUP_K_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, GROUP_K_MAX, k);
  if (agg < 0 || agg > 1) return fail(c, POI_EINVAL, "%s: agg must be 0 (mean) or 1 (least misery) (got %d)", who, agg);
  if (n < 0 || n_item <= 0 || n_grp < 0) return fail(c, POI_EINVAL, "%s: n < 0, n_item <= 0 or n_grp < 0", who);
  if ((ex_off == nullptr) != (ex == nullptr)) return fail(c, POI_EINVAL, "%s: ex_off and ex go together", who);
  return POI_OK;
}

int poi_group_topk(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                   const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                   const int32_t* g_off, const int32_t* g_mem, int32_t n_grp, int32_t agg, const int32_t* ex_off, const int32_t* ex, int32_t k,
                   int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (!c || !items || (!users && n > 0)) return fail(c, POI_EINVAL, "poi_group_topk: NULL ctx / users / items");
  int rc;
  if ((rc = group_check_args(c, "poi_group_topk", n, n_item, g_off, g_mem, n_grp, agg, ex_off, ex, k, idx_out))) return rc;
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_group_topk: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  const bool geo = wd != nullptr;
  if (geo && (!sts || !coords || !cphi || !thr || !last_poi)) return fail(c, POI_EINVAL, "poi_group_topk: the distance term needs sts / coords / cphi / thr / last_poi");
  if (geo && (n_dist <= 0 || !(dd > 0))) return fail(c, POI_EINVAL, "poi_group_topk: the distance term needs n_dist > 0 and dd > 0");
  if (is_f16(c, users)) return fail(c, POI_ENOTSUP, "poi_group_topk: users must be float32");
  if (n_grp == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::GroupArgs A = {};
  A.users = users; A.items = items; A.items_f16 = is_f16(c, items);
  A.n = n; A.n_item = n_item; A.dim = dim; A.k = k; A.n_grp = n_grp; A.agg = agg;
  if (geo) { A.wd = wd; A.sts = sts; A.coords = coords; A.cphi = cphi; A.thr = thr; A.last_poi = last_poi; A.n_dist = n_dist; A.bin_scale = (float)(12742.0 * 1000.0 / dd); }
  A.g_off = g_off; A.g_mem = g_mem; A.ex_off = ex_off; A.ex = ex;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  // few groups (live traffic): the item range is cut into slices so that the call fills the CUs; many groups: one workgroup per GROUP_GPT groups
  const int split = n_grp <= c->group_split_max;
  const int n_gtile = (n_grp + GROUP_GPT - 1) / GROUP_GPT, ntile = (n_item + 31) / 32;
  A.n_split = 1;
  if (split) {
    int s = c->group_grid > 0 ? c->group_grid : 2 * c->num_cu / n_gtile;
    if (c->group_grid <= 0 && s > ntile / 16) s = ntile / 16;      // (at least four item tiles per wave)
    if (c->group_grid <= 0 && s < 2) s = 2;
    A.n_split = s > GROUP_SPLIT_LIMIT ? GROUP_SPLIT_LIMIT : s;
    const size_t lists = (size_t)n_grp * A.n_split;
    if ((rc = ensure(c, c->group_ws, lists * (GROUP_K_MAX * (sizeof(float) + sizeof(int)) + sizeof(int)), st))) return rc;
    A.part_s = (float*)c->group_ws.p;
    A.part_i = (int*)(A.part_s + lists * GROUP_K_MAX);
    A.part_cnt = A.part_i + lists * GROUP_K_MAX;
  }
  c->plan.valid = 1; c->plan.group_path = split; c->plan.group_splits = split ? A.n_split : 0; c->plan.group_split_max = c->group_split_max;
  HIPCHK(c, poi::launch_group(A, st, &c->tm));
  return POI_OK;
}

int poi_group_topk_scores(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, const int32_t* g_off, const int32_t* g_mem, int32_t n_grp,
                          int32_t agg, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out,
                          void* stream) {
  if (!c || (!scores && n > 0)) return fail(c, POI_EINVAL, "poi_group_topk_scores: NULL ctx / scores");
  int rc;
  if ((rc = group_check_args(c, "poi_group_topk_scores", n, n_item, g_off, g_mem, n_grp, agg, ex_off, ex, k, idx_out))) return rc;
  if (n_grp == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::GroupArgs A = {};
  A.n = n; A.n_item = n_item; A.k = k; A.n_grp = n_grp; A.agg = agg; A.n_split = 1;
  A.g_off = g_off; A.g_mem = g_mem; A.ex_off = ex_off; A.ex = ex;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  HIPCHK(c, poi::launch_group_scores(scores, A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// fold-in of new users (foldin.hip)
int poi_foldin_bpr(poi_ctx* c, const float* items, int32_t n_item, int32_t dim, const int32_t* off, const int32_t* p, const int32_t* q,
                   int64_t q_epoch_stride, int32_t n, int32_t epochs, float alpha, float lambda, const float* w0, float* w_out,
                   float* loss_out, void* stream) {
  if (!c || !items || !w_out) return fail(c, POI_EINVAL, "poi_foldin_bpr: NULL ctx / items / w_out");
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_foldin_bpr: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  if (n < 0 || n_item <= 0 || epochs < 0 || q_epoch_stride < 0) return fail(c, POI_EINVAL, "poi_foldin_bpr: n < 0, n_item <= 0, epochs < 0 or q_epoch_stride < 0");
  if (n == 0) return POI_OK;
  if (!off || !p || !q) return fail(c, POI_EINVAL, "poi_foldin_bpr: NULL off / p / q");
  if ((w0 && is_f16(c, w0)) || is_f16(c, w_out)) return fail(c, POI_ENOTSUP, "poi_foldin_bpr: w0 / w_out must be float32");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::FoldinArgs A = {};
  A.items = items; A.items_f16 = is_f16(c, items);
  A.n = n; A.n_item = n_item; A.dim = dim; A.epochs = epochs;
  A.off = off; A.p = p; A.q = q; A.q_epoch_stride = q_epoch_stride;
  A.alpha = alpha; A.lambda = lambda;
  A.w0 = w0; A.w_out = w_out; A.loss_out = loss_out;
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  HIPCHK(c, poi::launch_foldin(A, st, &c->tm));
  return POI_OK;
}

// fold-in for the successive-POI models (foldin_seq.hip): the per-step scalars, then the generalised chain
static int foldin_terms_common(poi_ctx* c, const char* who, const int32_t* off, const int32_t* p, const int32_t* q, int64_t q_epoch_stride, int32_t n,
                               int64_t total, int32_t epochs, const double* c_out, poi::FoldinTermsArgs& A) {
  if (n < 0 || total < 0 || epochs < 0 || q_epoch_stride < 0) return fail(c, POI_EINVAL, "%s: n < 0, total < 0, epochs < 0 or q_epoch_stride < 0", who);
  if (total >= ((int64_t)1 << 31)) return fail(c, POI_ENOTSUP, "%s: at most 2^31 - 1 check-ins per call", who);
  if (q_epoch_stride != 0 && q_epoch_stride < total) return fail(c, POI_EINVAL, "%s: q_epoch_stride must be 0 or at least total", who);
  if (n == 0 || total == 0 || epochs == 0) return POI_OK;
  if (!off || !p || !q || !c_out) return fail(c, POI_EINVAL, "%s: NULL off / p / q / c_out", who);
  A.off = off; A.p = p; A.q = q; A.q_epoch_stride = q_epoch_stride; A.n = n; A.total = total;
  A.n_epoch = q_epoch_stride ? epochs : 1;
  return POI_OK;
}

int poi_foldin_terms_fpmc(poi_ctx* c, const poi_fpmc_params* P, const int32_t* off, const int32_t* p, const int32_t* q, int64_t q_epoch_stride,
                          int32_t n, int64_t total, int32_t epochs, double* c_out, void* stream) {
  if (!c || !P || !P->ia || !P->ai) return fail(c, POI_EINVAL, "poi_foldin_terms_fpmc: NULL ctx / params / ia / ai");
  if (is_f16(c, P->ia) || is_f16(c, P->ai)) return fail(c, POI_ENOTSUP, "FPMC-LR tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "poi_foldin_terms_fpmc: dim must be a multiple of 4 in [4, 256] (got %d)", P->dim);
  if (P->n_item <= 0) return fail(c, POI_EINVAL, "poi_foldin_terms_fpmc: n_item <= 0");
  poi::FoldinTermsArgs A = {};
  int rc = foldin_terms_common(c, "poi_foldin_terms_fpmc", off, p, q, q_epoch_stride, n, total, epochs, c_out, A);
  if (rc || !A.off) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  A.tab_pq = P->ia; A.tab_prev = P->ai; A.n_item = P->n_item; A.dim = P->dim; A.c_out = c_out;
  HIPCHK(c, poi::launch_foldin_terms(A, false, c->num_cu, st, &c->tm));
  return POI_OK;
}

int poi_foldin_terms_prme(poi_ctx* c, const poi_prme_params* P, const double* cordi, const int32_t* off, const int32_t* p, const int32_t* q,
                          int64_t q_epoch_stride, const int32_t* gap, const double* dist, int32_t n, int64_t total, int32_t epochs, int32_t threshold,
                          float cw, double* a_out, double* c_out, void* stream) {
  if (!c || !P || !P->ds) return fail(c, POI_EINVAL, "poi_foldin_terms_prme: NULL ctx / params / ds");
  if (is_f16(c, P->ds)) return fail(c, POI_ENOTSUP, "PRME tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 256) return fail(c, POI_ENOTSUP, "poi_foldin_terms_prme: dim must be a multiple of 4 in [4, 256] (got %d)", P->dim);
  if (P->n_item <= 0) return fail(c, POI_EINVAL, "poi_foldin_terms_prme: n_item <= 0");
  poi::FoldinTermsArgs A = {};
  int rc = foldin_terms_common(c, "poi_foldin_terms_prme", off, p, q, q_epoch_stride, n, total, epochs, c_out, A);
  if (rc || !A.off) return rc;
  if (!gap || !a_out || (!dist && !cordi)) return fail(c, POI_EINVAL, "poi_foldin_terms_prme: NULL gap / a_out, or neither dist nor cordi");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  A.tab_pq = P->ds; A.tab_prev = P->ds; A.n_item = P->n_item; A.dim = P->dim; A.c_out = c_out; A.a_out = a_out;
  A.gap = gap; A.dist = dist; A.cordi = cordi; A.thd = threshold; A.cw = cw;
  HIPCHK(c, poi::launch_foldin_terms(A, true, c->num_cu, st, &c->tm));
  return POI_OK;
}

int poi_foldin_pair(poi_ctx* c, const float* items, int32_t n_item, int32_t dim, int32_t form, int32_t first, const int32_t* off, const int32_t* p,
                    const int32_t* q, int64_t q_epoch_stride, const double* a, const double* cterm, int64_t c_epoch_stride, int32_t n, int32_t epochs,
                    float alpha, float lambda, const float* w0, float* w_out, float* loss_out, void* stream) {
  if (!c || !items || !w_out) return fail(c, POI_EINVAL, "poi_foldin_pair: NULL ctx / items / w_out");
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_foldin_pair: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  if (form != FOLDIN_FORM_DOT && form != FOLDIN_FORM_METRIC) return fail(c, POI_EINVAL, "poi_foldin_pair: form must be POI_FOLDIN_DOT or POI_FOLDIN_METRIC (got %d)", form);
  if (first != 0 && first != 1) return fail(c, POI_EINVAL, "poi_foldin_pair: first must be 0 or 1 (got %d)", first);
  if (n < 0 || n_item <= 0 || epochs < 0 || q_epoch_stride < 0 || c_epoch_stride < 0)
    return fail(c, POI_EINVAL, "poi_foldin_pair: n < 0, n_item <= 0, epochs < 0 or a negative epoch stride");
  if (n == 0) return POI_OK;
  if (!off || !p || !q) return fail(c, POI_EINVAL, "poi_foldin_pair: NULL off / p / q");
  if (is_f16(c, items) || (w0 && is_f16(c, w0)) || is_f16(c, w_out)) return fail(c, POI_ENOTSUP, "poi_foldin_pair: items / w0 / w_out must be float32");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::FoldinPairArgs A = {};
  A.items = items; A.n = n; A.n_item = n_item; A.dim = dim; A.epochs = epochs; A.form = form; A.first = first;
  A.off = off; A.p = p; A.q = q; A.q_epoch_stride = q_epoch_stride;
  A.a = form == FOLDIN_FORM_METRIC ? a : nullptr; A.c = cterm; A.c_epoch_stride = c_epoch_stride;
  A.alpha = alpha; A.lambda = lambda;
  A.w0 = w0; A.w_out = w_out; A.loss_out = loss_out;
  int rc;
  if ((rc = ensure(c, c->bad_ids, 64, st))) return rc;
  A.bad = (int*)c->bad_ids.p;
  A.dummy = (const double*)c->bad_ids.p + 4;      // (bytes 32 .. 39 of the counter's buffer: never written)
  HIPCHK(c, poi::launch_foldin_pair(A, st, &c->tm));
  return POI_OK;
}

int poi_topk(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, int32_t k, int32_t* idx_out, float* score_out,
             void* stream) {
  if (!c || !scores || !idx_out) return fail(c, POI_EINVAL, "poi_topk: NULL argument");
  if (k <= 0 || k > 64 || k > n_item) return fail(c, POI_ENOTSUP, "poi_topk supports 1 <= k <= min(64, n_item) (got %d)", k);
  if (n < 0) return fail(c, POI_EINVAL, "n < 0");
  if (n == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_topk_rows(scores, n, n_item, k, idx_out, score_out, (hipStream_t)stream));
  return POI_OK;
}

int poi_auc_preference(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t dim,
                       const int32_t* tp, const int32_t* tq, const int32_t* tm, int32_t len, uint8_t* out, void* stream) {
  if (!c || !users || !items || !tp || !tq || !tm || !out) return fail(c, POI_EINVAL, "poi_auc_preference: NULL argument");
  if (dim <= 0 || dim % 4 != 0) return fail(c, POI_ENOTSUP, "dim must be a positive multiple of 4");
  if (n < 0 || len < 0) return fail(c, POI_EINVAL, "bad sizes");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_auc(users, items, is_f16(c, items), n, dim, tp, tq, tm, len, out, (hipStream_t)stream));
  return POI_OK;
}

int poi_sumsq(poi_ctx* c, const float* x, int64_t n, double* out, void* stream) {
  if (!c || !x || !out || n < 0) return fail(c, POI_EINVAL, "poi_sumsq: bad argument");
  if (n == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (is_f16(c, x)) HIPCHK(c, poi::launch_sumsq_f16(x, n, out, (hipStream_t)stream));
  else HIPCHK(c, poi::launch_sumsq(x, n, out, (hipStream_t)stream));
  return POI_OK;
}

int poi_dist_prob(poi_ctx* c, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                  const float* sts, int32_t n, int32_t n_item, int32_t n_dist, double dd, float* prob_out, void* stream) {
  if (!c || !coords || !last_poi || !sts || !prob_out) return fail(c, POI_EINVAL, "poi_dist_prob: NULL argument");
  if ((cphi == nullptr) != (thr == nullptr)) return fail(c, POI_EINVAL, "poi_dist_prob: cphi and thr go together");
  if (n < 0 || n_item <= 0 || n_dist <= 0 || !(dd > 0)) return fail(c, POI_EINVAL, "bad sizes");
  HIPCHK(c, hipSetDevice(c->device));
  for (int32_t o = 0; o < n; o += 32768) {
    const int32_t m = n - o < 32768 ? n - o : 32768;
    c->tm.begin("dist_prob", (hipStream_t)stream);
    HIPCHK(c, poi::launch_dist_prob(coords, cphi, thr, last_poi + o, sts + (size_t)o * (n_dist + 1), m, n_item, n_dist, dd,
                                    prob_out + (size_t)o * n_item, (hipStream_t)stream));
    c->tm.end((hipStream_t)stream);
  }
  return POI_OK;
}

int poi_rank_metrics(poi_ctx* c, const int32_t* ranks, int32_t n, int32_t k, const int32_t* tes_p, const int32_t* tes_mask,
                     int32_t len_tes, const int32_t* at_nums, int32_t n_at, double* acc, void* stream) {
  if (!c || !ranks || !tes_p || !tes_mask || !at_nums || !acc) return fail(c, POI_EINVAL, "poi_rank_metrics: NULL argument");
  if (n < 0 || k <= 0 || len_tes <= 0 || n_at <= 0 || n_at > 8) return fail(c, POI_EINVAL, "poi_rank_metrics: bad sizes (n_at <= 8)");
  if (n == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_rank_metrics(ranks, n, k, tes_p, tes_mask, len_tes, at_nums, n_at, acc, (hipStream_t)stream));
  return POI_OK;
}

int poi_sample_negatives(poi_ctx* c, const int32_t* off, const int32_t* p, int32_t n_user, int32_t n_item, const int32_t* tes_p,
                         const int32_t* tes_mask, int32_t len_tes, uint64_t seed, int32_t* q_out, int32_t* tes_q_out, void* stream) {
  if (!c || !off || !p || !q_out) return fail(c, POI_EINVAL, "poi_sample_negatives: NULL argument");
  if (tes_q_out && (!tes_p || !tes_mask || len_tes <= 0)) return fail(c, POI_EINVAL, "poi_sample_negatives: test tables missing");
  if (n_user < 0 || n_item <= 0) return fail(c, POI_EINVAL, "bad sizes");
  if (n_user == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("sample_neg", (hipStream_t)stream);
  HIPCHK(c, poi::launch_sample_neg(off, p, n_user, n_item, tes_p, tes_mask, len_tes, seed, q_out, tes_q_out, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_neg_dist_bins(poi_ctx* c, const int32_t* off, const int32_t* p, const int32_t* q, int32_t n_user, const double* coords,
                      const double* cphi, const double* thr, int32_t n_dist, double dd, int32_t* dq_out, void* stream) {
  if (!c || !off || !p || !q || !coords || !cphi || !thr || !dq_out) return fail(c, POI_EINVAL, "poi_neg_dist_bins: NULL argument");
  if (n_user < 0 || n_dist <= 0 || !(dd > 0)) return fail(c, POI_EINVAL, "bad sizes");
  if (n_user == 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->tm.begin("neg_dist", (hipStream_t)stream);
  HIPCHK(c, poi::launch_neg_dist(off, p, q, n_user, coords, cphi, thr, n_dist, dd, dq_out, (hipStream_t)stream));
  c->tm.end((hipStream_t)stream);
  return POI_OK;
}

int poi_delta_make(poi_ctx* c, const float* cur, const float* base, float* delta, int64_t n, void* stream) {
  if (!c || !cur || !base || !delta || n < 0) return fail(c, POI_EINVAL, "poi_delta_make: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_delta_make(cur, base, delta, n, (hipStream_t)stream));
  return POI_OK;
}

int poi_delta_apply(poi_ctx* c, float* cur, const float* base, const float* delta_sum, int64_t n, void* stream) {
  if (!c || !cur || !base || !delta_sum || n < 0) return fail(c, POI_EINVAL, "poi_delta_apply: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_delta_apply(cur, base, delta_sum, n, (hipStream_t)stream));
  return POI_OK;
}

int poi_ctx_set_engine(poi_ctx* c, int engine) {
  if (!c || engine < 0 || engine > 4) return fail(c, POI_EINVAL, "engine must be 0 (auto), 1 (per-sequence), 2 (tile), 3 (tile, streaming recurrent kernels) or 4 (exact: float64)");
  c->engine = engine;
  return POI_OK;
}

int poi_ctx_set_f16_rounding(poi_ctx* c, int mode, uint32_t seed) {
  if (!c || mode < 0 || mode > 1) return fail(c, POI_EINVAL, "poi_ctx_set_f16_rounding: mode must be 0 (nearest) or 1 (stochastic)");
  c->f16_rounding = mode; c->sr_counter = seed;
  return POI_OK;
}

int poi_ctx_set_split_products(poi_ctx* c, int on) {
  if (!c || on < 0 || on > 1) return fail(c, POI_EINVAL, "poi_ctx_set_split_products: on must be 0 or 1");
  c->rec_split = on;
  return POI_OK;
}

int poi_ctx_set_exact_forward(poi_ctx* c, int on, int per_sequence_max) {
  if (!c || on < 0 || on > 1) return fail(c, POI_EINVAL, "poi_ctx_set_exact_forward: on must be 0 or 1");
  c->xfwd = on;
  if (per_sequence_max >= 0) c->xrec1_max = per_sequence_max;
  drop_graphs(c);
  return POI_OK;
}

int poi_ctx_set_option(poi_ctx* c, const char* name, int value) {
  if (!c || !name) return fail(c, POI_EINVAL, "poi_ctx_set_option: null argument");
  struct Opt { const char* name; int* p; int lo, hi; };
  const Opt opts[] = {{"forward_table_compact", &c->xcomp, 0, 1}, {"forward_table_compact_min", &c->xcomp_min, 0, 1 << 30}, {"head_split", &c->head3, 0, 1},
                      {"early_bins", &c->early_bins, 0, 1}, {"hot_bins", &c->hot_bins, 0, 1}, {"hybrid", &c->hybrid, 0, 1}, {"hybrid_min", &c->hyb_min, 0, 1 << 30}, {"hybrid_max", &c->hyb_max, 0, 1 << 30}, {"hybrid_force", &c->hyb_force, 0, 1 << 30},
                      {"cell_grid", &c->cell_grid, 0, 1 << 30}, {"vbpr_grid", &c->vbpr_grid, 0, 1 << 30}, {"session_tile_min", &c->sess_tile_min, 1, 1 << 30},
                      {"near_split_max", &c->near_split_max, 0, 1 << 30}, {"near_grid", &c->near_grid, 0, NEAR_SPLIT_LIMIT},
                      {"rank_grid", &c->rank_grid, 0, 1 << 30}, {"geoie_score_span", &c->geo_span, 0, 1 << 30},
                      {"group_split_max", &c->group_split_max, 0, 1 << 30}, {"group_grid", &c->group_grid, 0, GROUP_SPLIT_LIMIT}};
  for (const Opt& o : opts)
    if (!strcmp(name, o.name)) {
      if (value < o.lo || value > o.hi) return fail(c, POI_EINVAL, "poi_ctx_set_option: %s must be in [%d, %d] (got %d)", name, o.lo, o.hi, value);
      *o.p = value;
      drop_graphs(c);
      return POI_OK;
    }
  return fail(c, POI_EINVAL, "poi_ctx_set_option: unknown option '%s'", name);
}

int poi_ctx_set_small_launch(poi_ctx* c, int max_sequences) {
  if (!c || max_sequences < 0) return fail(c, POI_EINVAL, "poi_ctx_set_small_launch: max_sequences must be >= 0");
  c->rec1_max = max_sequences;
  return POI_OK;
}

int poi_ctx_set_regroup_min(poi_ctx* c, int min_sequences) {
  if (!c || min_sequences < 0) return fail(c, POI_EINVAL, "poi_ctx_set_regroup_min: min_sequences must be >= 0");
  c->bintab_min = min_sequences;
  return POI_OK;
}

int poi_ctx_set_one_sequence_path(poi_ctx* c, int on) {
  if (!c || on < 0 || on > 1) return fail(c, POI_EINVAL, "poi_ctx_set_one_sequence_path: on must be 0 or 1");
  c->one_path = on;
  return POI_OK;
}

int poi_ctx_set_topk_filter(poi_ctx* c, int on) {
  if (!c || on < 0 || on > 3) return fail(c, POI_EINVAL, "poi_ctx_set_topk_filter: on must be 0 (one-stage only), 1 (two-stage), 2 / 3 (two-stage, item-stationary GEO filter forced / forbidden)");
  c->topk_filter = on != 0;
  c->sf_items = on == 2 ? 1 : on == 3 ? 0 : -1;
  return POI_OK;
}

int poi_ctx_topk_filter_stats(poi_ctx* c, int64_t* users, int64_t* survivors, int64_t* tiles, int64_t* tiles_flagged) {
  if (!c || !users || !survivors || !tiles || !tiles_flagged) return fail(c, POI_EINVAL, "poi_ctx_topk_filter_stats: NULL argument");
  *users = c->last_two_n; *tiles = c->last_two_tiles; *survivors = 0; *tiles_flagged = 0;
  if (c->last_two_n <= 0) return POI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<int> cnt((size_t)c->last_two_n), fl((size_t)c->last_two_tiles);
  HIPCHK(c, hipMemcpy(cnt.data(), c->surv_cnt.p, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(fl.data(), c->tflag.p, sizeof(int) * fl.size(), hipMemcpyDeviceToHost));
  for (int v : cnt) *survivors += v;
  for (int v : fl) *tiles_flagged += v != 0;
  return POI_OK;
}

int poi_ctx_set_topk_seed(poi_ctx* c, const int32_t* seed_idx, int32_t k_seed) {
  if (!c || (seed_idx && (k_seed <= 0 || k_seed > 64))) return fail(c, POI_EINVAL, "poi_ctx_set_topk_seed: k_seed must be in [1, 64]");
  c->seed_idx = seed_idx; c->seed_k = seed_idx ? k_seed : 0;
  return POI_OK;
}

int poi_ctx_set_graph(poi_ctx* c, int on, int min_n, int max_n) {
  if (!c || on < 0 || on > 1 || min_n < 0 || max_n < min_n) return fail(c, POI_EINVAL, "poi_ctx_set_graph: on must be 0 / 1 and 0 <= min_n <= max_n");
  if (on && !c->cap) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->cap, hipStreamNonBlocking));
  }
  c->graph_mode = on; c->graph_min_n = min_n; c->graph_max_n = max_n;
  return POI_OK;
}

int64_t poi_ctx_graph_replays(const poi_ctx* c) { return c ? (int64_t)c->graph_replays : POI_EINVAL; }

int poi_ctx_last_plan(poi_ctx* c, const char* key, int64_t* value) {
  if (!c || !key || !value) return fail(c, POI_EINVAL, "poi_ctx_last_plan: NULL argument");
  const poi_ctx::LastPlan& R = c->plan;
  if (!R.valid) return fail(c, POI_EINVAL, "poi_ctx_last_plan: no training launch on this context yet");
  static const struct { const char* name; int poi_ctx::LastPlan::*f; } flags[] = {
      {"tile", &poi_ctx::LastPlan::tile}, {"one", &poi_ctx::LastPlan::one}, {"rec1", &poi_ctx::LastPlan::rec1}, {"xrec1", &poi_ctx::LastPlan::xrec1},
      {"hyb", &poi_ctx::LastPlan::hyb}, {"bintab", &poi_ctx::LastPlan::bintab}, {"ppoi", &poi_ctx::LastPlan::ppoi}, {"listed", &poi_ctx::LastPlan::listed},
      {"fwd_tab", &poi_ctx::LastPlan::fwd_tab}, {"xft", &poi_ctx::LastPlan::xft}, {"xcomp", &poi_ctx::LastPlan::xcomp},
      {"head_split", &poi_ctx::LastPlan::head_split}, {"efuse", &poi_ctx::LastPlan::efuse}, {"early_bins", &poi_ctx::LastPlan::early_bins},
      {"fork", &poi_ctx::LastPlan::fork}, {"cell_kernel", &poi_ctx::LastPlan::cell_kernel}, {"cell_grid", &poi_ctx::LastPlan::cell_grid},
      {"session_path", &poi_ctx::LastPlan::session_path}, {"session_tiles", &poi_ctx::LastPlan::session_tiles},
      {"session_tile_min", &poi_ctx::LastPlan::session_tile_min}, {"near_path", &poi_ctx::LastPlan::near_path},
      {"near_splits", &poi_ctx::LastPlan::near_splits}, {"near_split_max", &poi_ctx::LastPlan::near_split_max},
      {"rank_splits", &poi_ctx::LastPlan::rank_splits}, {"geoie_score_span", &poi_ctx::LastPlan::geoie_score_span},
      {"geoie_score_splits", &poi_ctx::LastPlan::geoie_score_splits}, {"group_path", &poi_ctx::LastPlan::group_path},
      {"group_splits", &poi_ctx::LastPlan::group_splits}, {"group_split_max", &poi_ctx::LastPlan::group_split_max}};
  for (const auto& e : flags)
    if (!strcmp(key, e.name)) { *value = R.*e.f; return POI_OK; }
  static const char* const hyb_keys[] = {"hyb_fwd_seq", "hyb_fwd_wg", "hyb_bwd_seq", "hyb_bwd_wg"};      // the order of TeArgs.hyb_dev
  for (int i = 0; i < 4; ++i) {
    if (strcmp(key, hyb_keys[i])) continue;
    if (!R.hyb) { *value = -1; return POI_OK; }
    if (R.ws_gen != c->te_ws_gen) return fail(c, POI_EINVAL, "poi_ctx_last_plan(\"%s\"): a later tile-engine launch may have reused the workspace", key);
    int v[4];
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(R.st));
    HIPCHK(c, hipMemcpy(v, R.hyb_dev, sizeof v, hipMemcpyDeviceToHost));
    *value = v[i];
    return POI_OK;
  }
  return fail(c, POI_EINVAL, "poi_ctx_last_plan: unknown key \"%s\"", key);
}
int64_t poi_ctx_take_bad_ids(poi_ctx* c, void* stream) {
  if (!c) return POI_EINVAL;
  if (!c->bad_ids.p) return 0;
  hipStream_t st = (hipStream_t)stream;
  int v = 0;
  if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync(&v, c->bad_ids.p, sizeof v, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) return fail(c, POI_EHIP, "poi_ctx_take_bad_ids: %s", hipGetErrorString(hipGetLastError()));
  if (v && (hipMemsetAsync(c->bad_ids.p, 0, sizeof v, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) return fail(c, POI_EHIP, "poi_ctx_take_bad_ids: reset failed");
  return v;
}

int poi_ctx_register_f16(poi_ctx* c, const void* ptr, int64_t bytes) {
  if (!c || !ptr || bytes <= 0) return fail(c, POI_EINVAL, "poi_ctx_register_f16: bad argument");
  for (auto& r : c->f16) if (r.first == (const char*)ptr) { r.second = (size_t)bytes; return POI_OK; }
  c->f16.emplace_back((const char*)ptr, (size_t)bytes);
  return POI_OK;
}

int poi_ctx_unregister_f16(poi_ctx* c, const void* ptr) {
  if (!c) return fail(c, POI_EINVAL, "NULL ctx");
  for (size_t i = 0; i < c->f16.size(); ++i) if (c->f16[i].first == (const char*)ptr) { c->f16.erase(c->f16.begin() + i); return POI_OK; }
  return POI_OK;
}

int poi_ctx_set_batch_cap(poi_ctx* c, float cap) {
  if (!c || !(cap >= 1.0f || cap == 0.0f)) return fail(c, POI_EINVAL, "batch cap must be >= 1 (1 = mean rule) or 0 (mini-batch rule)");
  c->batch_cap = cap;
  return POI_OK;
}

int poi_timing_enable(poi_ctx* c, int on) {
  if (!c) return fail(c, POI_EINVAL, "NULL ctx");
  c->tm.on = on != 0;
  c->tm.period = on > 1 ? on : 1; c->tm.count = 0; c->tm.active = true;
  return POI_OK;
}

int poi_timing_reset(poi_ctx* c) {
  if (!c) return fail(c, POI_EINVAL, "NULL ctx");
  HIPCHK(c, hipDeviceSynchronize());
  c->tm.clear();
  return POI_OK;
}

int poi_timing_get(poi_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
  if (!c || !kernel || !total_ms || !launches) return fail(c, POI_EINVAL, "poi_timing_get: NULL argument");
  HIPCHK(c, hipDeviceSynchronize());
  double tot = 0; int64_t n = 0;
  for (auto& r : c->tm.recs) {
    if (r.name != kernel) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { tot += ms; ++n; }
  }
  *total_ms = tot; *launches = n;
  return POI_OK;
}

int poi_selftest(poi_ctx* c, void* stream) {
  if (!c) return fail(c, POI_EINVAL, "NULL ctx");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure(c, c->st, 64, st);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->st.p, 0, 64, st));
  float* buf = (float*)c->st.p;
  int* flag = (int*)((char*)c->st.p + 32);
  HIPCHK(c, poi::launch_selftest(buf, flag, st));
  float hb[8]; int hf = -1;
  HIPCHK(c, hipMemcpyAsync(hb, buf, sizeof hb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&hf, flag, sizeof hf, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (hf != 0) return fail(c, POI_EHIP, "selftest: %d wave/block reduction mismatches", hf);
  for (int i = 0; i < 8; ++i) if (hb[i] != 256.0f) return fail(c, POI_EHIP, "selftest: float atomic count %g != 256", hb[i]);
  return POI_OK;
}

}  // extern "C"
