// C-ABI of libpoi_hip.so (see include/poi_hip.h): context, scratch ownership, argument checks,
// kernel dispatch.  No torch types, no host allocation handed to the caller.
#include "abi_internal.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {
thread_local std::string g_err;
}

int is_f16(const poi_ctx* c, const void* p) {
  if (!c || !p) return 0;
  for (auto& r : c->f16) if ((const char*)p >= r.first && (const char*)p < r.first + r.second) return 1;
  return 0;
}

int fail(poi_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  if (c) c->err = buf;
  return code;
}

// Grow-only zero-initialised device buffer.  Contents are all-zero after (re)allocation; users
// of gradient tables rely on that and restore the zeros themselves after each launch.
int ensure(poi_ctx* c, DevBuf& b, size_t bytes, hipStream_t st) {
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

int refuse_batch_cap0(poi_ctx* c) {
  if (c->batch_cap != 0.0f) return POI_OK;
  return fail(c, POI_ENOTSUP, "the mini-batch rule (batch cap 0) applies to poi_gru_step / poi_spatial_step only");
}

int bad_counter(poi_ctx* c, hipStream_t st, int** bad) {
  int rc = ensure(c, c->bad_ids, 64, st);      // (zero-filled at allocation)
  *bad = (int*)c->bad_ids.p;
  return rc;
}

int check_ex_pair(poi_ctx* c, const char* who, const void* ex_off, const void* ex, const char* verb) {
  if ((ex_off == nullptr) != (ex == nullptr)) return fail(c, POI_EINVAL, "%s: ex_off and ex %s together", who, verb);
  return POI_OK;
}

int check_geo_term(poi_ctx* c, const char* who, bool geo, bool ptrs_ok, const char* ptr_msg, int n_dist, double dd, float* bin_scale) {
  if (!ptrs_ok) return fail(c, POI_EINVAL, "%s: %s", who, ptr_msg);
  if (geo && (n_dist <= 0 || !(dd > 0))) return fail(c, POI_EINVAL, "%s: the distance term needs n_dist > 0 and dd > 0", who);
  *bin_scale = geo ? (float)(12742.0 * 1000.0 / dd) : 0.f;
  return POI_OK;
}

// c >= (1 - cos a) / 2 = sin^2(a / 2): a POI more than 2 asin(sqrt(c)) away in latitude is never within the radius (1e-6 relative margin)
double lat_band_deg(double c) { return c >= 1.0 ? 1e9 : 2.0 * asin(sqrt(c)) / 0.017453292519943295 * (1.0 + 1e-6) + 1e-9; }

void drop_graphs(poi_ctx* c) {
  for (auto& g : c->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
  c->graphs.clear(); c->seen_key.clear();
}

// The caller's float32 alpha / lambda are the nearest floats to short decimals (0.01, 0.001: prog_bpr_gru_spatial.py:66-67); the
// float64 engine takes the SHORTEST decimal that rounds to the given float - 0.01, not 0.00999999977648 - so that its step equals
// the float64 reference's to rounding, not to 2e-8.
double shortest_decimal(float x) {
  char buf[64];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)x);
    if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
  }
  return (double)x;
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
  if (const char* e = getenv("POI_TE_STREAM")) c->stream_hints = atoi(e) != 0;
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
  if (const char* e = getenv("POI_TE_XIDS_LDS")) c->xids_lds = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_XCOMP_MIN")) c->xcomp_min = atoi(e);
  if (const char* e = getenv("POI_TE_REC1")) c->rec1_max = atoi(e);
  if (const char* e = getenv("POI_TE_ONE")) c->one_path = atoi(e) != 0;
  if (const char* e = getenv("POI_TE_BINTAB_MIN")) c->bintab_min = atoi(e);
  if (const char* e = getenv("POI_CARNN_FAST")) c->carnn_fast = atoi(e) != 0;
  if (const char* e = getenv("POI_GRAPH")) c->graph_mode = atoi(e) != 0;
  if (const char* e = getenv("POI_TOPK_FILTER")) c->topk_filter = atoi(e) != 0;
  if (const char* e = getenv("POI_SF_ITEMS")) c->sf_items_env = atoi(e) != 0;
  if (const char* e = getenv("POI_SF_NSPLIT")) c->sf_nsplit = atoi(e);
  if (const char* e = getenv("POI_SCORE_DBG")) c->score_dbg = atoi(e);
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

int poi_ctx_destroy(poi_ctx* c) {
  if (!c) return POI_OK;
  (void)hipDeviceSynchronize();
  c->tm.clear();
  drop_graphs(c);
  if (c->cap) (void)hipStreamDestroy(c->cap);
  if (c->side2) { (void)hipStreamDestroy(c->side2); (void)hipEventDestroy(c->ev_h0); (void)hipEventDestroy(c->ev_h1); (void)hipEventDestroy(c->ev_h2); (void)hipEventDestroy(c->ev_h3); }
  if (c->side) { (void)hipStreamDestroy(c->side); (void)hipEventDestroy(c->ev_slots); (void)hipEventDestroy(c->ev_sorted); (void)hipEventDestroy(c->ev_bwd); (void)hipEventDestroy(c->ev_fin); (void)hipEventDestroy(c->ev_start); (void)hipEventDestroy(c->ev_pack); (void)hipEventDestroy(c->ev_hr0); (void)hipEventDestroy(c->ev_hr1); }
  delete c;      // frees every DevBuf member
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
  // (the 16-sequence tiles of te_rec_fwdx store G, H, RH non-temporally - large launches only: a small launch's rows stay on-die for te_rec_bwd, and a
  // row of dim 64 is half the bytes: stream_min counts sequences of dim 128; POI_TE_DBG bit 16384: plain stores, for A/B runs)
  A.stream_hints = (c->stream_hints && A.xfwd && D <= 128 && !A.xrec1 && !predict && (size_t)n * D >= (size_t)c->stream_min * 128 && !(A.dbg & 16384)) ? 1 : 0;
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
    // (the ids of a sequence's steps in LDS: the step capacity Tcap was sized with; 0 - in-loop loads - when switched off or when the table does not fit)
    A.xid_cap = (A.xft && c->xids_lds) ? poi::te_xfwd_ids_cap(D, predict ? T->max_len : (T->max_len > 1 ? T->max_len - 1 : 1), A.xrec1 != 0) : 0;
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
      R.fwd_tab = E.fwd_tab; R.xft = E.xft; R.xcomp = E.xcomp; R.xfwd_ids_lds = E.xid_cap > 0; R.stream_hints = one ? 0 : E.stream_hints; R.head_split = E.head_split; R.efuse = one ? 0 : E.efuse; R.early_bins = E.early_bins;
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
                             (uint64_t)E.fwd_tab, (uint64_t)E.xfwd, (uint64_t)E.xft, (uint64_t)E.xrec1, (uint64_t)E.xcomp, (uint64_t)(unsigned)E.xid_cap, (uint64_t)(unsigned)c->xcomp_min, (uint64_t)E.head_split, (uint64_t)(unsigned)c->xrec1_max, (uint64_t)E.ppoi, (uint64_t)one, (uint64_t)E.hyb, (uint64_t)E.efuse, (uint64_t)E.hot_early, (uint64_t)E.stream_hints};
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
    c->plan.valid = 1; c->plan.xfwd_ids_lds = E.xid_cap > 0;      // (the one plan value a predict launch records)
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
  const Opt opts[] = {{"forward_table_compact", &c->xcomp, 0, 1}, {"forward_table_compact_min", &c->xcomp_min, 0, 1 << 30}, {"xfwd_ids_lds", &c->xids_lds, 0, 1}, {"head_split", &c->head3, 0, 1},
                      {"early_bins", &c->early_bins, 0, 1}, {"hot_bins", &c->hot_bins, 0, 1}, {"stream_hints", &c->stream_hints, 0, 1}, {"stream_hints_min", &c->stream_min, 0, 1 << 30}, {"hybrid", &c->hybrid, 0, 1}, {"hybrid_min", &c->hyb_min, 0, 1 << 30}, {"hybrid_max", &c->hyb_max, 0, 1 << 30}, {"hybrid_force", &c->hyb_force, 0, 1 << 30},
                      {"cell_grid", &c->cell_grid, 0, 1 << 30}, {"vbpr_grid", &c->vbpr_grid, 0, 1 << 30}, {"session_tile_min", &c->sess_tile_min, 1, 1 << 30},
                      {"near_split_max", &c->near_split_max, 0, 1 << 30}, {"near_grid", &c->near_grid, 0, NEAR_SPLIT_LIMIT},
                      {"rank_grid", &c->rank_grid, 0, 1 << 30}, {"geoie_score_span", &c->geo_span, 0, 1 << 30},
                      {"group_split_max", &c->group_split_max, 0, 1 << 30}, {"group_grid", &c->group_grid, 0, GROUP_SPLIT_LIMIT},
                      {"route_split_max", &c->route_split_max, 0, 1 << 30}, {"route_grid", &c->route_grid, 0, ROUTE_SPLIT_LIMIT},
                      {"diverse_split_max", &c->diverse_split_max, 0, 1 << 30}, {"diverse_grid", &c->diverse_grid, 0, DIVERSE_SPLIT_LIMIT},
                      {"select_split_max", &c->select_split_max, 0, 1 << 30}, {"select_grid", &c->select_grid, 0, SELECT_SPLIT_LIMIT},
                      {"select_chunk_mb", &c->select_chunk_mb, 1, 1 << 20},
                      {"filter_split_max", &c->filter_split_max, 0, 1 << 30}, {"filter_grid", &c->filter_grid, 0, FILTER_SPLIT_LIMIT},
                      {"filter_gather_cost", &c->filter_gather_cost, 1, 1 << 20},
                      {"audience_split_max", &c->audience_split_max, 0, 1 << 30}, {"audience_grid", &c->audience_grid, 0, AUDIENCE_SPLIT_LIMIT},
                      {"similar_split_max", &c->similar_split_max, 0, 1 << 30}, {"similar_grid", &c->similar_grid, 0, SIMILAR_SPLIT_LIMIT},
                      {"similar_rows_max", &c->similar_rows_max, 0, SIMILAR_ROWS_MAX_LIMIT},
                      {"capped_split_max", &c->capped_split_max, 0, 1 << 30}, {"capped_grid", &c->capped_grid, 0, CAPPED_SPLIT_LIMIT},
                      {"capped_hist_kb", &c->capped_hist_kb, 1, 1 << 21},
                      {"labels_split_max", &c->labels_split_max, 0, 1 << 30}, {"labels_grid", &c->labels_grid, 0, LABELS_SPLIT_LIMIT},
                      {"labels_lds_kb", &c->labels_lds_kb, 0, LABELS_LDS_KB_MAX}, {"labels_ws_kb", &c->labels_ws_kb, 1, 1 << 30},
                      {"explain_start", &c->explain_start, 0, 1}};
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
      {"fwd_tab", &poi_ctx::LastPlan::fwd_tab}, {"xft", &poi_ctx::LastPlan::xft}, {"xcomp", &poi_ctx::LastPlan::xcomp}, {"xfwd_ids_lds", &poi_ctx::LastPlan::xfwd_ids_lds}, {"stream_hints", &poi_ctx::LastPlan::stream_hints},
      {"head_split", &poi_ctx::LastPlan::head_split}, {"efuse", &poi_ctx::LastPlan::efuse}, {"early_bins", &poi_ctx::LastPlan::early_bins},
      {"fork", &poi_ctx::LastPlan::fork}, {"cell_kernel", &poi_ctx::LastPlan::cell_kernel}, {"cell_grid", &poi_ctx::LastPlan::cell_grid},
      {"session_path", &poi_ctx::LastPlan::session_path}, {"session_tiles", &poi_ctx::LastPlan::session_tiles},
      {"session_tile_min", &poi_ctx::LastPlan::session_tile_min}, {"near_path", &poi_ctx::LastPlan::near_path},
      {"near_splits", &poi_ctx::LastPlan::near_splits}, {"near_split_max", &poi_ctx::LastPlan::near_split_max},
      {"rank_splits", &poi_ctx::LastPlan::rank_splits}, {"geoie_score_span", &poi_ctx::LastPlan::geoie_score_span},
      {"geoie_score_splits", &poi_ctx::LastPlan::geoie_score_splits}, {"group_path", &poi_ctx::LastPlan::group_path},
      {"group_splits", &poi_ctx::LastPlan::group_splits}, {"group_split_max", &poi_ctx::LastPlan::group_split_max},
      {"route_path", &poi_ctx::LastPlan::route_path}, {"route_splits", &poi_ctx::LastPlan::route_splits},
      {"diverse_path", &poi_ctx::LastPlan::diverse_path}, {"diverse_splits", &poi_ctx::LastPlan::diverse_splits},
      {"diverse_split_max", &poi_ctx::LastPlan::diverse_split_max},
      {"select_rows_per_chunk", &poi_ctx::LastPlan::select_rows_per_chunk}, {"select_chunks", &poi_ctx::LastPlan::select_chunks},
      {"select_path", &poi_ctx::LastPlan::select_path}, {"select_splits", &poi_ctx::LastPlan::select_splits},
      {"filter_path", &poi_ctx::LastPlan::filter_path}, {"filter_splits", &poi_ctx::LastPlan::filter_splits},
      {"filter_split_max", &poi_ctx::LastPlan::filter_split_max},
      {"audience_path", &poi_ctx::LastPlan::audience_path}, {"audience_splits", &poi_ctx::LastPlan::audience_splits},
      {"audience_split_max", &poi_ctx::LastPlan::audience_split_max},
      {"similar_path", &poi_ctx::LastPlan::similar_path}, {"similar_splits", &poi_ctx::LastPlan::similar_splits},
      {"similar_split_max", &poi_ctx::LastPlan::similar_split_max},
      {"capped_splits", &poi_ctx::LastPlan::capped_splits}, {"capped_split_max", &poi_ctx::LastPlan::capped_split_max},
      {"lists_path", &poi_ctx::LastPlan::lists_path},
      {"labels_splits", &poi_ctx::LastPlan::labels_splits}, {"labels_split_max", &poi_ctx::LastPlan::labels_split_max},
      {"labels_home", &poi_ctx::LastPlan::labels_home}, {"labels_chunks", &poi_ctx::LastPlan::labels_chunks},
      {"labels_rows_per_chunk", &poi_ctx::LastPlan::labels_rows_per_chunk},
      {"explain_columns", &poi_ctx::LastPlan::explain_columns}, {"explain_tiles", &poi_ctx::LastPlan::explain_tiles},
      {"explain_start", &poi_ctx::LastPlan::explain_start}};
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
