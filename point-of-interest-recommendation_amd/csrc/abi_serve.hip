// C-ABI of libpoi_hip.so (see include/poi_hip.h): everything that answers a query - scoring, top-K, ranks, sessions, fold-ins, metrics, samplers, deltas.
#include "abi_internal.h"
#include "score_plan.h"

#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

extern "C" {

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

// PRME scoring (prme.hip)
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
// scoring under the trained rule (geoie_score.hip): k == 0 writes the (n_rows, n_item) matrix, k > 0 the lists
static int geoie_score_common(poi_ctx* c, const char* who, const poi_geoie_params* P, const int32_t* off, const int32_t* p, const int32_t* mult,
                              const float* tu, const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min,
                              float* out, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out,
                              int32_t* count_out, void* stream) {
  int rc = geoie_check(c, P, who);
  if (rc) return rc;
  if (n_rows < 0) return fail(c, POI_EINVAL, "%s: n_rows < 0", who);
  if (!(d_min >= 0.0)) return fail(c, POI_EINVAL, "%s: d_min must be >= 0", who);
  if (int r = check_ex_pair(c, who, ex_off, ex)) return r;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
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
    if ((rc = carve_lists(c, c->geo_ws, st, A, (size_t)n_rows * A.n_split, GEO_K_MAX))) return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  HIPCHK(c, poi::launch_session(A, 0, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// leave-one-out attribution (explain.hip)
// ---------------------------------------------------------------------------------------------
int poi_explain_loo(poi_ctx* c, const poi_gru_params* P, const double* coords, const double* cphi, const double* thr, double dd,
                    const int32_t* h_off, const int32_t* h_ids, int64_t total, const int32_t* grp, const int32_t* g_off, int32_t n_group,
                    int32_t n, int32_t max_len, const int32_t* base_cols, const int32_t* var_cols, int32_t n_var, const int32_t* lists,
                    int32_t n_list, double* base, double* delta, double* h_out, double* sts_out, int32_t* last_out, void* stream) {
  if (!c || !P) return fail(c, POI_EINVAL, "poi_explain_loo: NULL ctx/params");
  if (!P->lt || !P->ui || !P->wh || !P->bi) return fail(c, POI_EINVAL, "poi_explain_loo: lt/ui/wh/bi must be non-NULL");
  const bool spatial = P->di != nullptr || P->n_dist != 0;
  int rc = session_check(c, P, spatial, "poi_explain_loo");
  if (rc) return rc;
  if (spatial && (!coords || !cphi || !thr || !P->wd || !(dd > 0))) return fail(c, POI_EINVAL, "poi_explain_loo: the spatial cell needs coords / cphi / thr / wd and dd > 0");
  if (n < 0 || n_group < 0 || n_var < 0 || total < 0 || max_len < 0) return fail(c, POI_EINVAL, "poi_explain_loo: n / n_group / n_var / total / max_len < 0");
  if (n_list <= 0 || n_list > EXPLAIN_C_MAX) return fail(c, POI_ENOTSUP, "poi_explain_loo supports 1 <= n_list <= %d (got %d)", EXPLAIN_C_MAX, n_list);
  const int xw = spatial ? 2 * P->dim : P->dim, NB = spatial ? P->n_dist + 1 : 1;
  if (!poi::explain_supported(P->dim, xw, NB, spatial ? 1 : 0))
    return fail(c, POI_ENOTSUP, "poi_explain_loo: dim must be a multiple of 16 in [16, 256] (got %d) and the tile must fit the LDS - build the model with pad_dim=True", P->dim);
  if (n == 0) return POI_OK;
  if (!h_off || !h_ids || !grp || !g_off || !base_cols || !lists || !base) return fail(c, POI_EINVAL, "poi_explain_loo: NULL h_off / h_ids / grp / g_off / base_cols / lists / base");
  if (n_var > 0 && (!var_cols || !delta || n_group <= 0)) return fail(c, POI_EINVAL, "poi_explain_loo: variants need var_cols / delta and n_group > 0");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::ExplainArgs A = poi::ExplainArgs{};
  A.lt = P->lt; A.lt_f16 = is_f16(c, P->lt);
  A.di = P->di; A.ui = P->ui; A.wh = P->wh; A.bi = P->bi; A.vs = P->vs; A.bs = P->bs; A.wd = P->wd;
  A.n_item = P->n_item; A.n_dist = spatial ? P->n_dist : 0; A.dim = P->dim; A.xw = xw; A.spatial = spatial ? 1 : 0;
  A.coords = coords; A.cphi = cphi; A.thr = thr; A.dd = dd;
  A.h_off = h_off; A.h_ids = h_ids; A.total = total; A.grp = grp; A.g_off = g_off; A.n_group = n_group; A.n = n;
  A.base_cols = base_cols; A.var_cols = var_cols; A.n_var = n_var; A.start_mode = c->explain_start;
  A.nck = max_len > 16 ? (max_len - 1) / 16 : 0;
  A.lists = lists; A.C = n_list; A.base = base; A.delta = delta; A.h_out = h_out; A.sts_out = sts_out; A.last_out = last_out;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  if ((rc = carve(c, c->explain_ws, st, [&](Carver& W) {
         A.rowbad = (int*)W.bytes(sizeof(int) * (size_t)n);
         A.ck = (double*)W.bytes(sizeof(double) * (size_t)n * (size_t)A.nck * (size_t)A.dim);
       })))
    return rc;
  c->plan.valid = 1; c->plan.explain_columns = n + n_var; c->plan.explain_tiles = (n + 15) / 16 + (n_var + 15) / 16; c->plan.explain_start = c->explain_start;
  HIPCHK(c, poi::launch_explain(A, st, &c->tm));
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
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

// POI2Vec scoring (poi2vec.hip)
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
  const size_t ns = (size_t)(axis == 0 ? P->n_item : n_batch);
  if ((rc = carve(c, c->pv_sc, st, [&](Carver& W) {
        A.cl = (double*)W.bytes(sizeof(double) * (rows * P->dim)); A.zf = (double*)W.bytes(sizeof(double) * (rows * P->n_node)); A.rp = (double*)W.bytes(sizeof(double) * (rows * NL));
        A.ssum = (double*)W.bytes(sizeof(double) * (ns)); A.smax = (float*)W.bytes(sizeof(float) * (ns)); A.logit = (float*)W.bytes(sizeof(float) * ((size_t)n_batch * P->n_item));
      }))) return rc;
  A.out = out;                                     // NULL for the top-K: the scores are not stored
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
  if (c) if (int r = check_ex_pair(c, "poi_poi2vec_topk_ex", ex_off, ex, "come")) return r;
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
  int* bad;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  const int n_span = (n_item + P2V_FOLD_SPAN - 1) / P2V_FOLD_SPAN;
  const size_t per_user = sizeof(double) * (size_t)n_span * (size_t)(dim + 2);
  size_t uc = P2V_FOLD_PART_BYTES / per_user / P2V_FOLD_USERS * P2V_FOLD_USERS;
  if (uc < P2V_FOLD_USERS) uc = P2V_FOLD_USERS;
  if (uc > (size_t)n) uc = (size_t)n;
  poi::FoldP2vArgs A = {};
  if ((rc = carve(c, c->pv_fold, st, [&](Carver& W) {
        A.w = (double*)W.bytes(sizeof(double) * uc * dim); A.tbar = (double*)W.bytes(sizeof(double) * uc * dim);
        A.flag = (int*)W.bytes(sizeof(int) * uc); A.part = (double*)W.bytes(per_user * uc);
      }))) return rc;
  A.wl = wl; A.n_item = n_item; A.dim = dim; A.epochs = epochs; A.n_span = n_span; A.tgt = tgt; A.alpha = alpha; A.lambda = lambda; A.bad = bad;
  for (size_t r0 = 0; r0 < (size_t)n; r0 += uc) {
    A.n = (int)((size_t)n - r0 < uc ? (size_t)n - r0 : uc);
    A.off = off + r0;
    A.w0 = w0 ? w0 + r0 * dim : nullptr; A.w_out = w_out + r0 * dim; A.loss_out = loss_out ? loss_out + r0 * epochs : nullptr;
    HIPCHK(c, poi::launch_foldin_p2v(A, st, &c->tm));
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
  // plan: every decision of the call (score_plan.h), from its shape and the context's settings alone
  ScoreShape S = {};
  S.n = n; S.n_item = n_item; S.dim = dim; S.k = k; S.all_scores = scores != nullptr; S.seed_k = seed_idx ? seed_k : 0;
  S.dist = U ? (!U->bins ? SCORE_DIST_GEO : U->bin_bytes == 1 ? SCORE_DIST_BINS8 : SCORE_DIST_BINS16) : prob ? SCORE_DIST_PROB : SCORE_DIST_NONE;
  S.n_dist = U ? U->n_dist : 0;
  // (item-stationary filter: poi_ctx_set_topk_filter(2 / 3) first, then POI_SF_ITEMS, then the shape)
  const ScoreSettings C = {c->num_cu, c->score_variant, c->topk_filter, c->sf_items >= 0 ? c->sf_items : c->sf_items_env, c->sf_nsplit};
  const ScorePlan P = plan_score(S, C);
  // allocate: all of the call's buffers, before the first launch
  struct { DevBuf& b; size_t bytes; } const need[] = {
      {c->items_pk, P.b_items_pk}, {c->cand_s, P.b_cand_s}, {c->cand_i, P.b_cand_i}, {c->gbound, P.b_gbound}, {c->pre_idx, P.b_pre_idx}, {c->pre_sc, P.b_pre_sc},
      {c->items_pk16, P.b_items_pk16}, {c->inorm, P.b_inorm}, {c->surv_cnt, P.b_surv_cnt}, {c->surv_idx, P.b_surv_idx}, {c->surv_sc, P.b_surv_sc}, {c->tflag, P.b_tflag},
      {c->users_pk16, P.b_users_pk16}, {c->ubound, P.b_ubound}, {c->ugeo, P.b_ugeo}};
  for (const auto& e : need) if (int rc = ensure(c, e.b, e.bytes, st)) return rc;
  // launch
  const int n_utile = (n + 31) / 32, n_pad = n_utile * 32, ntile = (n_item + 31) / 32;
  poi::ScoreArgs A;
  memset(&A, 0, sizeof A);
  A.users = users; A.items = items; A.items_f16 = is_f16(c, items); A.n = n; A.n_item = n_item; A.dim = dim; A.wd = wd; A.prob = prob;
  A.scores = scores; A.k = k; A.idx_out = idx_out; A.score_out = score_out;
  if (U) { A.ulptai = U->bins; A.bin_bytes = U->bin_bytes; A.sts = U->sts; A.n_dist = U->n_dist; }
  if (U && !U->bins) { A.geo = 1; A.coords = U->coords; A.cphi = U->cphi; A.thr = U->thr; A.last_poi = U->last_poi; A.dd = U->dd; }
  A.dbg = c->score_dbg;
  A.n_split = P.n_split;
  if (P.variant) A.items_packed = (float4*)c->items_pk.p;
  // one-stage kernel of the plan's variant + merge of the per-range lists, on the item table X describes
  auto one_stage = [&](const poi::ScoreArgs& X) -> int {
    if (P.variant == 2) HIPCHK(c, poi::launch_score_geo_stream(X, st, &c->tm));
    else if (P.variant == 1) HIPCHK(c, poi::launch_score_packed(X, st, &c->tm));
    else HIPCHK(c, poi::launch_score(X, st, &c->tm));
    if (k > 0) HIPCHK(c, poi::launch_topk_merge(X, X.n_split, n_pad, st));
    return POI_OK;
  };
  if (k > 0) { A.cand_score = (float*)c->cand_s.p; A.cand_idx = (int*)c->cand_i.p; }
  if (P.gbound) {
    HIPCHK(c, hipMemsetAsync(c->gbound.p, 0, sizeof(unsigned) * (size_t)n_pad, st));
    A.gbound = (unsigned*)c->gbound.p;
  }
  if (P.seeded) {
    c->tm.begin("topk_seed", st);
    HIPCHK(c, poi::launch_topk_seed(A, seed_idx, seed_k, st));
    c->tm.end(st);
    A.seeded = 1;
  }
  if (P.pre == SCORE_PRE_PREFIX) {
    // the one-stage kernel on a prefix of the table -> bounds.  (X is taken before A learns of the two-stage buffers: with a tile_flag the
    // one-stage kernel would only run flagged tiles)
    poi::ScoreArgs X = A;
    X.n_item = P.sub_tiles * 32; X.bins_ntile = ntile; X.n_split = P.pre_split;
    X.idx_out = (int*)c->pre_idx.p; X.score_out = (float*)c->pre_sc.p;
    if (int rc = one_stage(X)) return rc;
    HIPCHK(c, poi::launch_topk_bound(X.score_out, n, k, A.gbound, st));
    A.seeded = 1;
  }
  if (P.two_stage) {
    // f16 filter pass + exact float32 rescoring of the survivors (score_filter.hip); the one-stage kernel below then only runs the user
    // tiles whose survivor lists overflowed (A.tile_flag)
    HIPCHK(c, hipMemsetAsync(c->surv_cnt.p, 0, sizeof(int) * (size_t)n_pad, st));
    HIPCHK(c, hipMemsetAsync(c->tflag.p, 0, sizeof(int) * (size_t)n_utile, st));
    A.items_packed16 = (const uint4*)c->items_pk16.p; A.inorm = (const float2*)c->inorm.p;
    A.surv_cnt = (int*)c->surv_cnt.p; A.surv_idx = (int*)c->surv_idx.p; A.surv_sc = (float*)c->surv_sc.p; A.tile_flag = (int*)c->tflag.p;
    A.n_cu = c->num_cu;
    if (P.items) { A.users_packed16 = (uint4*)c->users_pk16.p; A.ubound = (float4*)c->ubound.p; A.ugeo = (double*)c->ugeo.p; }
    if (P.pre == SCORE_PRE_MAXPASS) {
      HIPCHK(c, poi::launch_score_maxpass(A, P, st, &c->tm));
      A.seeded = 1;
    }
    HIPCHK(c, poi::launch_score_two_stage(A, P, st, &c->tm));
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
  float bin_scale;
  int rc;
  if ((rc = check_ex_pair(c, "poi_score_topk_near", ex_off, ex))) return rc;
  if ((rc = check_geo_term(c, "poi_score_topk_near", geo, geo == (sts != nullptr) && geo == (thr != nullptr), "wd, sts and thr go together", n_dist, dd, &bin_scale))) return rc;
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
  A.wd = wd; A.sts = sts; A.thr = thr; A.n_dist = geo ? n_dist : 0; A.bin_scale = bin_scale;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  // few rows (live traffic): every row's band is cut into slices so that the call fills the CUs; many rows: one workgroup per row
  const SplitPlan sp = plan_split(n, n, c->near_split_max, c->near_grid, 4, c->num_cu, INT_MAX, 2, NEAR_SPLIT_LIMIT);
  A.n_split = sp.n_split;
  if (sp.split && (rc = carve_lists(c, c->near_ws, st, A, (size_t)n * A.n_split, NEAR_K_MAX))) return rc;
  c->plan.valid = 1; c->plan.near_path = sp.split; c->plan.near_splits = sp.split ? A.n_split : 0; c->plan.near_split_max = c->near_split_max;
  HIPCHK(c, poi::launch_near(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// The operand block of the families that walk tiles of users . items (poi::TileOperands: rank.hip, group.hip, route.hip, diverse.hip):
// the checks each of them makes on the users / items / distance-term arguments and the exclusion pair, then the block itself, the
// half-table flag, the metres-per-bin factor and the context's counter of rejected rows included.  Selects the context's device.
static int tile_operands(poi_ctx* c, const char* who, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                         const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist,
                         double dd, const int32_t* ex_off, const int32_t* ex, hipStream_t st, poi::TileOperands* out) {
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, dim);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  const bool geo = wd != nullptr;
  float bin_scale;
  int rc;
  if ((rc = check_ex_pair(c, who, ex_off, ex))) return rc;
  if ((rc = check_geo_term(c, who, geo, !geo || (sts && coords && cphi && thr && last_poi), "the distance term needs sts / coords / cphi / thr / last_poi", n_dist, dd, &bin_scale))) return rc;
  if (is_f16(c, users)) return fail(c, POI_ENOTSUP, "%s: users must be float32", who);
  HIPCHK(c, hipSetDevice(c->device));
  poi::TileOperands& T = *out;
  T = poi::TileOperands{};
  T.users = users; T.items = items; T.items_f16 = is_f16(c, items);
  T.n = n; T.n_item = n_item; T.dim = dim;
  if (geo) { T.wd = wd; T.sts = sts; T.coords = coords; T.cphi = cphi; T.thr = thr; T.last_poi = last_poi; T.n_dist = n_dist; T.bin_scale = bin_scale; }
  T.ex_off = ex_off; T.ex = ex;
  return bad_counter(c, st, &T.bad);
}

// ---------------------------------------------------------------------------------------------
// exact target ranks (rank.hip)
static int rank_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* tgt, const int32_t* tmask, int32_t len_t,
                      const int32_t* ex_off, const int32_t* ex, const int32_t* rank_out) {
  if (!tgt || !tmask || !rank_out) return fail(c, POI_EINVAL, "%s: NULL tgt / tmask / rank_out", who);
  if (len_t <= 0 || len_t > RANK_LT_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= len_t <= %d (got %d)", who, RANK_LT_MAX, len_t);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if (int r = check_ex_pair(c, who, ex_off, ex)) return r;
  return POI_OK;
}

int poi_score_rank(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                   const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                   const int32_t* tgt, const int32_t* tmask, int32_t len_t, const int32_t* ex_off, const int32_t* ex, int32_t* rank_out,
                   float* score_out, int32_t* count_out, void* stream) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "poi_score_rank: NULL ctx / users / items");
  int rc;
  if ((rc = rank_check(c, "poi_score_rank", n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, "poi_score_rank", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (n == 0) return POI_OK;
  poi::RankArgs A = {};
  put_operands(A, T);
  A.len_t = len_t; A.tgt = tgt; A.tmask = tmask;
  A.rank_out = rank_out; A.score_out = score_out; A.count_out = count_out;
  const int n_utile = (n + 31) / 32, ntile = (n_item + 31) / 32;
  if ((rc = ensure(c, c->rank_ws, sizeof(poi::RankTgt) * (size_t)n_utile * 32 * RANK_LT_MAX, st))) return rc;
  A.tl = (poi::RankTgt*)c->rank_ws.p;
  // item ranges, one wave each (split_plan.h): "rank_grid" caps them, the 16-bit per-lane counters set the floor
  A.n_split = plan_wave_ranges(n_utile, ntile, c->num_cu, c->rank_grid, RANK_TILES_MAX);
  c->plan.valid = 1; c->plan.rank_splits = A.n_split;
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
  int* bad;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  c->tm.begin("rank_scores", st);
  HIPCHK(c, poi::launch_rank_scores(scores, n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out, count_out, bad, st));
  c->tm.end(st);
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// candidate generation (select.hip)
static int select_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, int32_t k, const int32_t* ex_off, const int32_t* ex,
                        const int32_t* idx_out) {
  if (!idx_out) return fail(c, POI_EINVAL, "%s: NULL idx_out", who);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if (k <= 0 || k > SELECT_K_MAX || k > n_item)
    return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= min(%d, n_item = %d) (got %d)", who, SELECT_K_MAX, n_item, k);
  return check_ex_pair(c, who, ex_off, ex);
}

// the slices of a call of n rows: few rows cut each row's id range so that the call fills the CUs (a slice keeps >= 2048 ids)
static SplitPlan select_plan(const poi_ctx* c, int n, int n_item) {
  return plan_split(n, n, c->select_split_max, c->select_grid, 4, c->num_cu, n_item / 2048 > 1 ? n_item / 2048 : 1, 1, SELECT_SPLIT_LIMIT);
}

// the workspace of `per` rows: histograms, state, candidate slots
static int select_carve(poi_ctx* c, poi::SelectArgs& A, int per, int k, hipStream_t st) {
  return carve(c, c->select_ws, st, [&](Carver& W) {
    A.hist = (int*)W.bytes(sizeof(int) * (size_t)per * SELECT_BINS);
    A.state = (int*)W.bytes(sizeof(int) * (size_t)per * SELECT_STATE_INTS);
    A.cand = (unsigned long long*)W.bytes(sizeof(unsigned long long) * (size_t)per * k);
  });
}

// the selection over score rows that are on the device, SELECT_ROWS_MAX rows per launch sequence; no host synchronisation in between
static int select_run(poi_ctx* c, const float* scores, int n, int n_item, int64_t ld, int k, const int32_t* ex_off, const int32_t* ex,
                      int32_t* idx_out, float* score_out, int32_t* count_out, int n_split, int* bad, hipStream_t st) {
  poi::SelectArgs A = {};
  A.n_item = n_item; A.ld = ld; A.k = k; A.n_split = n_split; A.ex = ex; A.bad = bad;
  const int per = n < SELECT_ROWS_MAX ? n : SELECT_ROWS_MAX;
  if (int rc = select_carve(c, A, per, k, st)) return rc;
  for (int o = 0; o < n; o += per) {
    A.n = n - o < per ? n - o : per;
    A.scores = scores + (size_t)o * (size_t)ld;
    A.ex_off = ex_off ? ex_off + o : nullptr;
    A.idx_out = idx_out + (size_t)o * k;
    A.score_out = score_out ? score_out + (size_t)o * k : nullptr;
    A.count_out = count_out ? count_out + o : nullptr;
    HIPCHK(c, poi::launch_select(A, st, &c->tm));
  }
  return POI_OK;
}

// item ranges, one wave each: poi_score_rank's rule (split_plan.h) without its cap and floor
static int score_rows_split(const poi_ctx* c, int n, int n_item) { return plan_wave_ranges((n + 31) / 32, (n_item + 31) / 32, c->num_cu, 0, 0); }

int poi_score_rows(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                   const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                   float* scores_out, int64_t ld, void* stream) {
  if (!c || !users || !items || !scores_out) return fail(c, POI_EINVAL, "poi_score_rows: NULL ctx / users / items / scores_out");
  if (ld < n_item) return fail(c, POI_EINVAL, "poi_score_rows: ld must be >= n_item");
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  int rc;
  if ((rc = tile_operands(c, "poi_score_rows", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, nullptr, nullptr, st, &T))) return rc;
  if (n == 0) return POI_OK;
  poi::ScoreRowsArgs A = {};
  put_operands(A, T);
  A.out = scores_out; A.ld = ld; A.n_split = score_rows_split(c, n, n_item);
  HIPCHK(c, poi::launch_score_rows(A, st, &c->tm));
  return POI_OK;
}

int poi_topk_select(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, int64_t ld, int32_t k, const int32_t* ex_off, const int32_t* ex,
                    int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (!c || !scores) return fail(c, POI_EINVAL, "poi_topk_select: NULL ctx / scores");
  int rc;
  if ((rc = select_check(c, "poi_topk_select", n, n_item, k, ex_off, ex, idx_out))) return rc;
  if (ld < n_item) return fail(c, POI_EINVAL, "poi_topk_select: ld must be >= n_item");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int* bad;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  const SplitPlan sp = select_plan(c, n, n_item);
  c->plan.valid = 1; c->plan.select_path = sp.split; c->plan.select_splits = sp.split ? sp.n_split : 0;
  c->plan.select_rows_per_chunk = n; c->plan.select_chunks = 1;
  const long span = c->tm.span_begin("topk_select", st);
  rc = select_run(c, scores, n, n_item, ld, k, ex_off, ex, idx_out, score_out, count_out, sp.n_split, bad, st);
  c->tm.span_end(span, st);
  return rc;
}

int poi_score_candidates(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                         const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist,
                         double dd, int32_t k, const int32_t* ex_off, const int32_t* ex, int32_t* idx_out, float* score_out, int32_t* count_out,
                         void* stream) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "poi_score_candidates: NULL ctx / users / items");
  int rc;
  if ((rc = select_check(c, "poi_score_candidates", n, n_item, k, ex_off, ex, idx_out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, "poi_score_candidates", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (n == 0) return POI_OK;
  // a whole number of 32-row tiles at a time, as many as fit "select_chunk_mb" (at least one tile)
  const int64_t ld = ((int64_t)n_item + 31) / 32 * 32;
  int64_t fit = ((int64_t)c->select_chunk_mb << 20) / (ld * 4) / 32 * 32;
  if (fit < 32) fit = 32;
  const int rows = (int)(fit < ((int64_t)n + 31) / 32 * 32 ? fit : ((int64_t)n + 31) / 32 * 32);
  float* sc_rows = nullptr;
  if ((rc = carve(c, c->select_sc, st, [&](Carver& W) { sc_rows = (float*)W.bytes(sizeof(float) * (size_t)rows * (size_t)ld); }))) return rc;
  {                                                 // both workspaces grow (and synchronise) before the first launch, not between chunks
    poi::SelectArgs S = {};
    const int top = rows < n ? rows : n;
    if ((rc = select_carve(c, S, top < SELECT_ROWS_MAX ? top : SELECT_ROWS_MAX, k, st))) return rc;
  }
  const SplitPlan sp = select_plan(c, n, n_item);
  c->plan.valid = 1; c->plan.select_path = sp.split; c->plan.select_splits = sp.split ? sp.n_split : 0;
  c->plan.select_rows_per_chunk = rows; c->plan.select_chunks = (n + rows - 1) / rows;
  const long span = c->tm.span_begin("score_candidates", st);
  for (int o = 0; o < n; o += rows) {
    const int m = n - o < rows ? n - o : rows;
    poi::ScoreRowsArgs A = {};
    put_operands(A, T);
    A.users = users + (size_t)o * dim; A.n = m;
    if (wd) { A.sts = sts + (size_t)o * (n_dist + 1); A.last_poi = last_poi + o; }
    A.out = sc_rows; A.ld = ld; A.n_split = score_rows_split(c, m, n_item);
    HIPCHK(c, poi::launch_score_rows(A, st, &c->tm));
    const long sel = c->tm.span_begin("topk_select", st);
    rc = select_run(c, sc_rows, m, n_item, ld, k, ex_off ? ex_off + o : nullptr, ex, idx_out + (size_t)o * k,
                    score_out ? score_out + (size_t)o * k : nullptr, count_out ? count_out + o : nullptr, sp.n_split, T.bad, st);
    c->tm.span_end(sel, st);
    if (rc) return rc;
  }
  c->tm.span_end(span, st);
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// re-ranking (rerank.hip)
int poi_score_lists_chunk(void) { return RERANK_CHUNK; }

static int lists_check(poi_ctx* c, const char* who, int32_t n, const int32_t* cand, int32_t n_cand) {
  if (!cand) return fail(c, POI_EINVAL, "%s: NULL cand", who);
  if (n < 0 || n_cand < 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_cand < 0", who);
  return POI_OK;
}

// the scoring launch of a call whose workspace is carved: the grid, the plan record
static int score_lists_run(poi_ctx* c, const poi::TileOperands& T, const int32_t* cand_off, const int32_t* cand, int32_t n_cand, int* flag, float* out,
                           hipStream_t st) {
  poi::ScoreListsArgs A = {};
  put_operands(A, T);
  A.cand_off = cand_off; A.cand = cand; A.n_cand = n_cand; A.flag = flag; A.out = out;
  if (cand_off) {
    // workgroups per row: 16 per CU over the call, no more than the chunks of the call's entries; a row's further chunks go round
    const int chunks = (n_cand + RERANK_CHUNK - 1) / RERANK_CHUNK;
    int want = (c->num_cu * 16 + T.n - 1) / T.n;
    if (want > chunks) want = chunks;
    A.n_split = want < 1 ? 1 : want;
  } else {
    // list ranges per 32-row tile, one wave each: 8 waves per CU over the call (poi_score_rows' rule), at least one 32-candidate tile each
    const int n_utile = (T.n + 31) / 32, ntile = (n_cand + 31) / 32;
    int want = (c->num_cu * 8 + n_utile - 1) / n_utile;
    if (want > ntile) want = ntile;
    A.n_split = want < 1 ? 1 : want;
  }
  c->plan.valid = 1; c->plan.lists_path = cand_off ? 0 : 1;
  HIPCHK(c, poi::launch_score_lists(A, st, &c->tm));
  return POI_OK;
}

static int rerank_check(poi_ctx* c, const char* who, const int32_t* cand_off, int32_t n_cand, int32_t k, const int32_t* idx_out) {
  if (!idx_out) return fail(c, POI_EINVAL, "%s: NULL idx_out", who);
  if (k <= 0 || k > RERANK_LEN_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, RERANK_LEN_MAX, k);
  if (!cand_off && n_cand > RERANK_LEN_MAX) return fail(c, POI_ENOTSUP, "%s supports a shared list of at most %d entries (got %d)", who, RERANK_LEN_MAX, n_cand);
  return POI_OK;
}

static int rerank_run(poi_ctx* c, const int32_t* cand_off, const int32_t* cand, int32_t n, int32_t n_cand, const float* score, const float* prior,
                      double w_score, double w_prior, const int* flag, int32_t k, int32_t* idx_out, float* score_out, int32_t* pos_out,
                      int32_t* count_out, int* bad, hipStream_t st) {
  poi::RerankListsArgs A = {};
  A.cand_off = cand_off; A.cand = cand; A.n = n; A.n_cand = n_cand; A.score = score; A.prior = prior; A.w_score = w_score; A.w_prior = w_prior;
  A.flag = flag; A.k = k; A.idx_out = idx_out; A.score_out = score_out; A.pos_out = pos_out; A.count_out = count_out; A.bad = bad;
  const int longest = n_cand < RERANK_LEN_MAX ? n_cand : RERANK_LEN_MAX;
  A.p_max = 1;
  while (A.p_max < longest) A.p_max <<= 1;
  HIPCHK(c, poi::launch_rerank_lists(A, st, &c->tm));
  return POI_OK;
}

int poi_score_lists(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                    const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                    const int32_t* cand_off, const int32_t* cand, int32_t n_cand, float* score_out, void* stream) {
  if (!c || !users || !items || !score_out) return fail(c, POI_EINVAL, "poi_score_lists: NULL ctx / users / items / score_out");
  int rc;
  if ((rc = lists_check(c, "poi_score_lists", n, cand, n_cand))) return rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, "poi_score_lists", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, nullptr, nullptr, st, &T))) return rc;
  if (n == 0 || n_cand == 0) return POI_OK;
  int* flag = nullptr;
  if ((rc = carve(c, c->rerank_ws, st, [&](Carver& W) { flag = (int*)W.bytes(sizeof(int) * (size_t)(cand_off ? n : 1)); }))) return rc;
  return score_lists_run(c, T, cand_off, cand, n_cand, flag, score_out, st);
}

int poi_rerank_lists(poi_ctx* c, const int32_t* cand_off, const int32_t* cand, int32_t n, int32_t n_cand, const float* score, const float* prior,
                     double w_score, double w_prior, int32_t k, int32_t* idx_out, float* score_out, int32_t* pos_out, int32_t* count_out,
                     void* stream) {
  if (!c || !score) return fail(c, POI_EINVAL, "poi_rerank_lists: NULL ctx / score");
  int rc;
  if ((rc = lists_check(c, "poi_rerank_lists", n, cand, n_cand))) return rc;
  if ((rc = rerank_check(c, "poi_rerank_lists", cand_off, n_cand, k, idx_out))) return rc;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int* bad;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  return rerank_run(c, cand_off, cand, n, n_cand, score, prior, w_score, w_prior, nullptr, k, idx_out, score_out, pos_out, count_out, bad, st);
}

int poi_rerank(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
               const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
               const int32_t* cand_off, const int32_t* cand, int32_t n_cand, const float* prior, double w_score, double w_prior, int32_t k,
               int32_t* idx_out, float* score_out, int32_t* pos_out, int32_t* count_out, void* stream) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "poi_rerank: NULL ctx / users / items");
  int rc;
  if ((rc = lists_check(c, "poi_rerank", n, cand, n_cand))) return rc;
  if ((rc = rerank_check(c, "poi_rerank", cand_off, n_cand, k, idx_out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, "poi_rerank", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, nullptr, nullptr, st, &T))) return rc;
  if (n == 0) return POI_OK;
  // the scores between the two stages live in the context; the stages follow each other on the stream, the host does not wait in between
  int* flag = nullptr;
  float* sc = nullptr;
  const size_t n_sc = cand_off ? (size_t)n_cand : (size_t)n * (size_t)n_cand;
  if ((rc = carve(c, c->rerank_ws, st, [&](Carver& W) {
         flag = (int*)W.bytes(sizeof(int) * (size_t)(cand_off ? n : 1));
         sc = (float*)W.bytes(sizeof(float) * (n_sc ? n_sc : 1));
       })))
    return rc;
  const long span = c->tm.span_begin("rerank", st);
  if (n_cand > 0) {
    if ((rc = score_lists_run(c, T, cand_off, cand, n_cand, flag, sc, st))) return rc;
  } else {
    c->plan.valid = 1; c->plan.lists_path = cand_off ? 0 : 1;
  }
  rc = rerank_run(c, cand_off, cand, n, n_cand, sc, prior, w_score, w_prior, n_cand > 0 ? flag : nullptr, k, idx_out, score_out, pos_out, count_out, T.bad, st);
  c->tm.span_end(span, st);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// group recommendation (group.hip)
static int group_check_args(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* g_off, const int32_t* g_mem, int32_t n_grp,
                            int32_t agg, const int32_t* ex_off, const int32_t* ex, int32_t k, const int32_t* idx_out) {
  if (!g_off || !g_mem || !idx_out) return fail(c, POI_EINVAL, "%s: NULL g_off / g_mem / idx_out", who);
  if (k <= 0 || k > GROUP_K_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, GROUP_K_MAX, k);
  if (agg < 0 || agg > 1) return fail(c, POI_EINVAL, "%s: agg must be 0 (mean) or 1 (least misery) (got %d)", who, agg);
  if (n < 0 || n_item <= 0 || n_grp < 0) return fail(c, POI_EINVAL, "%s: n < 0, n_item <= 0 or n_grp < 0", who);
  if (int r = check_ex_pair(c, who, ex_off, ex)) return r;
  return POI_OK;
}

int poi_group_topk(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                   const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                   const int32_t* g_off, const int32_t* g_mem, int32_t n_grp, int32_t agg, const int32_t* ex_off, const int32_t* ex, int32_t k,
                   int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (!c || !items || (!users && n > 0)) return fail(c, POI_EINVAL, "poi_group_topk: NULL ctx / users / items");
  int rc;
  if ((rc = group_check_args(c, "poi_group_topk", n, n_item, g_off, g_mem, n_grp, agg, ex_off, ex, k, idx_out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, "poi_group_topk", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (n_grp == 0) return POI_OK;
  poi::GroupArgs A = {};
  put_operands(A, T);
  A.k = k; A.n_grp = n_grp; A.agg = agg; A.g_off = g_off; A.g_mem = g_mem;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  // few groups (live traffic): the item range is cut into slices so that the call fills the CUs (at least four item tiles per wave);
  // many groups: one workgroup per GROUP_GPT groups
  const int n_gtile = (n_grp + GROUP_GPT - 1) / GROUP_GPT, ntile = (n_item + 31) / 32;
  const SplitPlan sp = plan_split(n_grp, n_gtile, c->group_split_max, c->group_grid, 2, c->num_cu, ntile / 16, 2, GROUP_SPLIT_LIMIT);
  A.n_split = sp.n_split;
  if (sp.split && (rc = carve_lists(c, c->group_ws, st, A, (size_t)n_grp * A.n_split, GROUP_K_MAX))) return rc;
  c->plan.valid = 1; c->plan.group_path = sp.split; c->plan.group_splits = sp.split ? A.n_split : 0; c->plan.group_split_max = c->group_split_max;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  HIPCHK(c, poi::launch_group_scores(scores, A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// audience recommendation (audience.hip)
static int audience_operands(poi_ctx* c, const char* who, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                             const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr,
                             const int32_t* last_poi, int32_t n_dist, double dd, const int32_t* pois, int32_t n_q, const int32_t* ex_off,
                             const int32_t* ex, hipStream_t st, poi::AudienceArgs* A) {
  if (!c || !items || (!users && n > 0)) return fail(c, POI_EINVAL, "%s: NULL ctx / users / items", who);
  if (n_q < 0 || (!pois && n_q > 0)) return fail(c, POI_EINVAL, "%s: n_q < 0 or NULL pois", who);
  if (wd && n_dist > AUDIENCE_NDIST_MAX) return fail(c, POI_ENOTSUP, "%s supports n_dist <= %d with the distance term (got %d)", who, AUDIENCE_NDIST_MAX, n_dist);
  poi::TileOperands T;
  if (int rc = tile_operands(c, who, users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, &T)) return rc;
  *A = poi::AudienceArgs{};
  put_operands(*A, T);
  A->pois = pois; A->n_q = n_q;
  // few queries (live traffic: a few POIs against every user): the rows are cut into slices so that the call fills the CUs; many: one
  // workgroup per 32-query block
  const SplitPlan sp = audience_plan(n_q, n, c->audience_split_max, c->audience_grid, c->num_cu);
  A->n_split = sp.n_split;
  if (n_q > 0) {
    c->plan.valid = 1; c->plan.audience_path = sp.split; c->plan.audience_splits = sp.split ? sp.n_split : 0;
    c->plan.audience_split_max = c->audience_split_max;
  }
  return POI_OK;
}

int poi_score_audience(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                       const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                       const int32_t* pois, int32_t n_q, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out,
                       int32_t* count_out, void* stream) {
  if (c && !idx_out) return fail(c, POI_EINVAL, "poi_score_audience: NULL idx_out");
  if (c && (k <= 0 || k > AUDIENCE_K_MAX)) return fail(c, POI_ENOTSUP, "poi_score_audience supports 1 <= k <= %d (got %d)", AUDIENCE_K_MAX, k);
  hipStream_t st = (hipStream_t)stream;
  poi::AudienceArgs A;
  int rc;
  if ((rc = audience_operands(c, "poi_score_audience", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, pois, n_q,
                              ex_off, ex, st, &A))) return rc;
  if (n_q == 0) return POI_OK;
  A.k = k; A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if (c->plan.audience_path && (rc = carve_lists(c, c->audience_ws, st, A, (size_t)n_q * A.n_split, AUDIENCE_K_MAX))) return rc;
  HIPCHK(c, poi::launch_audience(A, st, &c->tm));
  return POI_OK;
}

int poi_audience_rows(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                      const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                      const int32_t* pois, int32_t n_q, float* scores_out, int64_t ld, void* stream) {
  if (c && !scores_out && n_q > 0 && n > 0) return fail(c, POI_EINVAL, "poi_audience_rows: NULL scores_out");
  if (c && ld < n) return fail(c, POI_EINVAL, "poi_audience_rows: ld must be >= n");
  hipStream_t st = (hipStream_t)stream;
  poi::AudienceArgs A;
  if (int rc = audience_operands(c, "poi_audience_rows", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, pois, n_q,
                                 nullptr, nullptr, st, &A)) return rc;
  if (n_q == 0 || n == 0) return POI_OK;
  A.rows_out = scores_out; A.ld = ld;
  HIPCHK(c, poi::launch_audience_rows(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// similar rows (similar.hip)
int poi_row_inv_norms(poi_ctx* c, const float* x, int32_t n, int32_t dim, double* inv_out, void* stream) {
  if (!c || !x || (!inv_out && n > 0)) return fail(c, POI_EINVAL, "poi_row_inv_norms: NULL ctx / x / inv_out");
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_row_inv_norms: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  if (n < 0) return fail(c, POI_EINVAL, "poi_row_inv_norms: n < 0");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, poi::launch_row_inv_norms(x, is_f16(c, x), n, dim, inv_out, st, &c->tm));
  return POI_OK;
}

// the checks and the argument block poi_similar_topk and poi_similar_rows share; inv_norm NULL: the norms go to the context's workspace
static int similar_operands(poi_ctx* c, const char* who, const float* x, int32_t n, int32_t dim, const double* coords, const double* cphi,
                            double geo_weight, double scale_km, const double* inv_norm, const int32_t* queries, int32_t n_q, const int32_t* ex_off,
                            const int32_t* ex, hipStream_t st, poi::SimilarArgs* A, long* span = nullptr) {
  if (!c || !x) return fail(c, POI_EINVAL, "%s: NULL ctx / x", who);
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, dim);
  if (n <= 0) return fail(c, POI_EINVAL, "%s: n <= 0", who);
  if (n_q < 0 || (!queries && n_q > 0)) return fail(c, POI_EINVAL, "%s: n_q < 0 or NULL queries", who);
  if (!(geo_weight >= 0.0 && geo_weight < 1.0)) return fail(c, POI_EINVAL, "%s: geo_weight must lie in [0, 1) (got %g)", who, geo_weight);
  if (!(scale_km > 0.0)) return fail(c, POI_EINVAL, "%s: scale_km must be positive (got %g)", who, scale_km);
  if (geo_weight > 0.0 && (!coords || !cphi)) return fail(c, POI_EINVAL, "%s: geo_weight > 0 needs coords / cphi", who);
  if (int rc = check_ex_pair(c, who, ex_off, ex)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  *A = poi::SimilarArgs{};
  A->x = x; A->x_f16 = is_f16(c, x); A->n = n; A->dim = dim;
  if (geo_weight > 0.0) { A->coords = coords; A->cphi = cphi; }
  A->g = geo_weight; A->omg = 1.0 - geo_weight; A->scale_km = scale_km;
  A->queries = queries; A->n_q = n_q; A->ex_off = ex_off; A->ex = ex; A->count_bad = 1; A->n_split = 1;
  if (int rc = bad_counter(c, st, &A->bad)) return rc;
  if (n_q == 0) return POI_OK;
  if (span) *span = c->tm.span_begin("similar_topk", st);      // the call; inside it the norms, the walk and the merge / the rows and the selection
  if (!inv_norm) {                                  // (no cache is kept: none can go stale)
    if (int rc = ensure(c, c->similar_inv, sizeof(double) * (size_t)n, st)) return rc;
    HIPCHK(c, poi::launch_row_inv_norms(x, A->x_f16, n, dim, (double*)c->similar_inv.p, st, &c->tm));
    inv_norm = (const double*)c->similar_inv.p;
  }
  A->inv = inv_norm;
  return POI_OK;
}

int poi_similar_topk(poi_ctx* c, const float* x, int32_t n, int32_t dim, const double* coords, const double* cphi, double geo_weight,
                     double scale_km, const double* inv_norm, const int32_t* queries, int32_t n_q, const int32_t* ex_off, const int32_t* ex,
                     int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  if (c && !idx_out) return fail(c, POI_EINVAL, "poi_similar_topk: NULL idx_out");
  if (c && (k <= 0 || k > SIMILAR_K_MAX)) return fail(c, POI_ENOTSUP, "poi_similar_topk supports 1 <= k <= %d (got %d)", SIMILAR_K_MAX, k);
  hipStream_t st = (hipStream_t)stream;
  // the plan first: the workspaces grow (and may synchronise) before the first launch
  const int64_t ld = ((int64_t)(n > 0 ? n : 1) + 31) / 32 * 32;
  const long long rows_fit = c ? ((long long)c->select_chunk_mb << 20) / (ld * 4) : 0;
  const SimilarPlan P = c ? similar_plan(n_q, n, k, c->similar_rows_max, rows_fit, c->similar_split_max, c->similar_grid, c->num_cu) : SimilarPlan{0, 1};
  float* sc_rows = nullptr;
  poi::SimilarArgs A;
  int rc;
  if (c && n > 0 && n_q > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    if (P.path == 2) {
      if ((rc = carve(c, c->similar_sc, st, [&](Carver& W) { sc_rows = (float*)W.bytes(sizeof(float) * (size_t)n_q * (size_t)ld); }))) return rc;
      poi::SelectArgs S = {};
      if ((rc = select_carve(c, S, n_q < SELECT_ROWS_MAX ? n_q : SELECT_ROWS_MAX, k, st))) return rc;
    }
  }
  long span = -1;
  if ((rc = similar_operands(c, "poi_similar_topk", x, n, dim, coords, cphi, geo_weight, scale_km, inv_norm, queries, n_q, ex_off, ex, st, &A, &span))) return rc;
  if (n_q == 0) return POI_OK;
  A.k = k; A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out; A.n_split = P.n_split;
  c->plan.valid = 1; c->plan.similar_path = P.path; c->plan.similar_splits = P.n_split > 1 || P.path == 1 ? P.n_split : 0;
  c->plan.similar_split_max = c->similar_split_max;
  if (P.path == 2) {
    A.rows_out = sc_rows; A.ld = ld; A.count_bad = 0;
    HIPCHK(c, poi::launch_similar_rows(A, st, &c->tm));
    const SplitPlan sp = select_plan(c, n_q, n);
    const long sel = c->tm.span_begin("topk_select", st);
    rc = select_run(c, sc_rows, n_q, n, ld, k, ex_off, ex, idx_out, score_out, count_out, sp.n_split, A.bad, st);
    c->tm.span_end(sel, st);
    if (rc) return rc;
    HIPCHK(c, poi::launch_similar_fix_counts(A, st));
  } else {
    if (P.path == 1 && (rc = carve_lists(c, c->similar_ws, st, A, (size_t)n_q * A.n_split, SIMILAR_K_MAX))) return rc;
    HIPCHK(c, poi::launch_similar(A, st, &c->tm));
  }
  c->tm.span_end(span, st);
  return POI_OK;
}

int poi_similar_rows(poi_ctx* c, const float* x, int32_t n, int32_t dim, const double* coords, const double* cphi, double geo_weight,
                     double scale_km, const double* inv_norm, const int32_t* queries, int32_t n_q, float* scores_out, int64_t ld, void* stream) {
  if (c && !scores_out && n_q > 0) return fail(c, POI_EINVAL, "poi_similar_rows: NULL scores_out");
  if (c && ld < n) return fail(c, POI_EINVAL, "poi_similar_rows: ld must be >= n");
  hipStream_t st = (hipStream_t)stream;
  poi::SimilarArgs A;
  if (int rc = similar_operands(c, "poi_similar_rows", x, n, dim, coords, cphi, geo_weight, scale_km, inv_norm, queries, n_q, nullptr, nullptr, st, &A)) return rc;
  if (n_q == 0) return POI_OK;
  const SplitPlan sp = similar_split(n_q, n, c->similar_split_max, c->similar_grid, c->num_cu);
  A.n_split = sp.n_split; A.rows_out = scores_out; A.ld = ld;
  c->plan.valid = 1; c->plan.similar_path = sp.split; c->plan.similar_splits = sp.split ? sp.n_split : 0; c->plan.similar_split_max = c->similar_split_max;
  HIPCHK(c, poi::launch_similar_rows(A, st, &c->tm));
  return POI_OK;
}

int poi_similar_nearest(poi_ctx* c, const float* items, int32_t n_item, int32_t dim, const double* coords, const double* cphi, double geo_weight,
                        double scale_km, const int32_t* lists, int32_t n, int32_t k, const int32_t* h_off, const int32_t* h_ids, int32_t* pos_out,
                        double* sim_out, void* stream) {
  if (!c) return fail(c, POI_EINVAL, "poi_similar_nearest: NULL ctx");
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "poi_similar_nearest: n < 0 or n_item <= 0");
  if (k <= 0 || k > SIMILAR_K_MAX) return fail(c, POI_ENOTSUP, "poi_similar_nearest supports 1 <= k <= %d (got %d)", SIMILAR_K_MAX, k);
  if (!(geo_weight >= 0.0 && geo_weight <= 1.0)) return fail(c, POI_EINVAL, "poi_similar_nearest: geo_weight must lie in [0, 1] (got %g)", geo_weight);
  if (!(scale_km > 0.0)) return fail(c, POI_EINVAL, "poi_similar_nearest: scale_km must be positive (got %g)", scale_km);
  if (geo_weight > 0.0 && (!coords || !cphi)) return fail(c, POI_EINVAL, "poi_similar_nearest: geo_weight > 0 needs coords / cphi");
  if (geo_weight < 1.0) {
    if (!items) return fail(c, POI_EINVAL, "poi_similar_nearest: geo_weight < 1 needs items");
    if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "poi_similar_nearest: dim must be a multiple of 4 in [4, 256] (got %d)", dim);
  }
  if (n > 0 && (!lists || !h_off || !h_ids || !pos_out)) return fail(c, POI_EINVAL, "poi_similar_nearest: NULL lists / h_off / h_ids / pos_out");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::NearestArgs A = {};
  if (geo_weight < 1.0) { A.items = items; A.items_f16 = is_f16(c, items); A.dim = dim; }
  if (geo_weight > 0.0) { A.coords = coords; A.cphi = cphi; }
  A.n_item = n_item; A.geo_weight = geo_weight; A.scale_km = scale_km;
  A.lists = lists; A.n = n; A.k = k; A.h_off = h_off; A.h_ids = h_ids; A.pos_out = pos_out; A.sim_out = sim_out;
  if (int rc = bad_counter(c, st, &A.bad)) return rc;
  HIPCHK(c, poi::launch_similar_nearest(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// route recommendation (route.hip)
int poi_route_expand(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                     const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                     const int32_t* path, int32_t path_stride, int32_t path_len, const int32_t* ex_off, const int32_t* ex, int32_t rows_per_list,
                     const int32_t* live, int32_t b, int32_t* idx_out, float* score_out, double* lse_out, int32_t* count_out, void* stream) {
  if (!c || !users || !items || !idx_out || !score_out || !lse_out) return fail(c, POI_EINVAL, "poi_route_expand: NULL ctx / users / items / idx_out / score_out / lse_out");
  if (b <= 0 || b > ROUTE_B_MAX) return fail(c, POI_ENOTSUP, "poi_route_expand supports 1 <= b <= %d (got %d)", ROUTE_B_MAX, b);
  if (path_len < 0 || path_len > ROUTE_T_MAX) return fail(c, POI_ENOTSUP, "poi_route_expand supports 0 <= path_len <= %d (got %d)", ROUTE_T_MAX, path_len);
  if (path_len > 0 && (!path || path_stride < path_len)) return fail(c, POI_EINVAL, "poi_route_expand: path_len > 0 needs path and path_stride >= path_len");
  if (rows_per_list <= 0) return fail(c, POI_EINVAL, "poi_route_expand: rows_per_list must be positive (got %d)", rows_per_list);
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  int rc;
  if ((rc = tile_operands(c, "poi_route_expand", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (n == 0) return POI_OK;
  poi::RouteArgs A = {};
  put_operands(A, T);
  A.b = b; A.path = path; A.path_stride = path_stride; A.path_len = path_len;
  A.rows_per_list = rows_per_list; A.live = live;
  A.idx_out = idx_out; A.score_out = score_out; A.lse_out = lse_out; A.count_out = count_out;
  // few rows (live traffic: one user's 1 .. 8 hypotheses): the item range is cut over workgroups so that the call fills the CUs, and a
  // second kernel finishes the rows; many rows: one workgroup per 32-row tile, which finishes its own rows.  (A wave walks whole item blocks.)
  const int n_utile = (n + 31) / 32, ntile = (n_item + 31) / 32;
  A.n_blk = (ntile + ROUTE_LSE_TILES - 1) / ROUTE_LSE_TILES;
  const SplitPlan sp = plan_split(n, n_utile, c->route_split_max, c->route_grid, 2, c->num_cu, (A.n_blk + ROUTE_NWAVE - 1) / ROUTE_NWAVE, 1, ROUTE_SPLIT_LIMIT);
  A.n_split = sp.n_split; A.finish = !sp.split;
  const size_t rows = (size_t)n_utile * 32, lists = rows * A.n_split * ROUTE_NWAVE;
  if ((rc = carve(c, c->route_ws, st, [&](Carver& W) {
        A.part_s = (float*)W.bytes(sizeof(float) * lists * ROUTE_B_MAX);
        A.part_i = (int*)W.bytes(sizeof(int) * lists * ROUTE_B_MAX);
        A.part_lse = (double*)W.bytes(sizeof(double) * rows * A.n_blk * 2);
        A.row_st = (int*)W.bytes(sizeof(int) * rows);
        A.row_cnt = (int*)W.bytes(sizeof(int) * rows);
      })))
    return rc;
  c->plan.valid = 1; c->plan.route_path = sp.split; c->plan.route_splits = sp.split ? A.n_split : 0;
  HIPCHK(c, poi::launch_route_expand(A, st, &c->tm));
  return POI_OK;
}

int poi_route_merge(poi_ctx* c, const int32_t* idx, const float* score, const double* lse, const double* total_in, const int32_t* n_live,
                    int32_t n_slot, int32_t n_par, int32_t b, int32_t* parent_out, int32_t* poi_out, double* total_out, double* steplp_out,
                    int32_t* nlive_out, void* stream) {
  if (!c || !idx || !score || !lse || !total_in || !parent_out || !poi_out || !total_out)
    return fail(c, POI_EINVAL, "poi_route_merge: NULL ctx / idx / score / lse / total_in / parent_out / poi_out / total_out");
  if (b <= 0 || b > ROUTE_B_MAX || n_par <= 0 || n_par > ROUTE_B_MAX) return fail(c, POI_ENOTSUP, "poi_route_merge supports 1 <= b, n_par <= %d (got %d, %d)", ROUTE_B_MAX, b, n_par);
  if (n_slot < 0) return fail(c, POI_EINVAL, "poi_route_merge: n_slot < 0");
  if (n_slot == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::RouteMergeArgs A = {};
  A.idx = idx; A.score = score; A.lse = lse; A.total_in = total_in; A.n_live = n_live;
  A.n_slot = n_slot; A.n_par = n_par; A.b = b;
  A.parent_out = parent_out; A.poi_out = poi_out; A.total_out = total_out; A.steplp_out = steplp_out; A.nlive_out = nlive_out;
  HIPCHK(c, poi::launch_route_merge(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// diversified recommendation (diverse.hip)
// stage 1's arguments: its own limits around the operand block
static int diverse_pool_check(poi_ctx* c, const char* who, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                              const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr,
                              const int32_t* last_poi, int32_t n_dist, double dd, const int32_t* ex_off, const int32_t* ex, int32_t pool,
                              hipStream_t st, poi::TileOperands* T) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "%s: NULL ctx / users / items", who);
  if (pool <= 0 || pool > DIVERSE_POOL_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= pool <= %d (got %d)", who, DIVERSE_POOL_MAX, pool);
  if (int rc = tile_operands(c, who, users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, st, T)) return rc;
  if (wd && n_dist > DIVERSE_NDIST_MAX) return fail(c, POI_ENOTSUP, "%s supports n_dist <= %d (got %d)", who, DIVERSE_NDIST_MAX, n_dist);
  return POI_OK;
}

static int diverse_rerank_check(poi_ctx* c, const char* who, int32_t n, int32_t pool, const void* items, int32_t n_item, int32_t dim,
                                const double* coords, const double* cphi, int32_t k, double trade, double geo_weight, double scale_km,
                                const int32_t* idx_out) {
  if (!c || !idx_out) return fail(c, POI_EINVAL, "%s: NULL ctx / idx_out", who);
  if (k <= 0 || k > DIVERSE_K_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, DIVERSE_K_MAX, k);
  if (pool < k || pool > DIVERSE_POOL_MAX) return fail(c, POI_ENOTSUP, "%s supports k <= pool <= %d (got pool %d, k %d)", who, DIVERSE_POOL_MAX, pool, k);
  if (!(trade >= 0.0 && trade <= 1.0)) return fail(c, POI_EINVAL, "%s: trade must lie in [0, 1] (got %g)", who, trade);
  if (!(geo_weight >= 0.0 && geo_weight <= 1.0)) return fail(c, POI_EINVAL, "%s: geo_weight must lie in [0, 1] (got %g)", who, geo_weight);
  if (!(scale_km > 0.0)) return fail(c, POI_EINVAL, "%s: scale_km must be positive (got %g)", who, scale_km);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if (geo_weight > 0.0 && (!coords || !cphi)) return fail(c, POI_EINVAL, "%s: geo_weight > 0 needs coords / cphi", who);
  if (geo_weight < 1.0) {
    if (!items) return fail(c, POI_EINVAL, "%s: geo_weight < 1 needs items", who);
    if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, dim);
  }
  return POI_OK;
}

// stage 1 into (pool_idx, pool_score), or - both null - into the context's workspace, whose pieces come back through the same pointers
static int diverse_pool_run(poi_ctx* c, const poi::TileOperands& T, int32_t pool, int32_t** pool_idx, float** pool_score, int32_t* count_out,
                            hipStream_t st) {
  poi::DiverseArgs A = {};
  put_operands(A, T);
  A.k = pool; A.count_out = count_out;
  const int n = T.n;
  // few rows (live traffic): the item range of every 32-row tile is cut into slices so that the call fills the CUs (at least four item
  // tiles per wave); many rows: one workgroup per tile
  const int n_utile = (n + 31) / 32, ntile = (T.n_item + 31) / 32;
  const SplitPlan sp = plan_split(n, n_utile, c->diverse_split_max, c->diverse_grid, 2, c->num_cu, ntile / 16, 2, DIVERSE_SPLIT_LIMIT);
  const int split = sp.split;
  A.n_split = sp.n_split;
  int rc;
  const bool own = *pool_idx == nullptr;
  const size_t lists = split ? (size_t)n * A.n_split : 0;
  if ((rc = carve(c, c->diverse_ws, st, [&](Carver& W) {
        if (own) { *pool_idx = (int32_t*)W.bytes(sizeof(int32_t) * (size_t)n * pool); *pool_score = (float*)W.bytes(sizeof(float) * (size_t)n * pool); }
        if (split) {
          A.part_s = (float*)W.bytes(sizeof(float) * lists * DIVERSE_POOL_MAX);
          A.part_i = (int*)W.bytes(sizeof(int) * lists * DIVERSE_POOL_MAX);
          A.part_cnt = (int*)W.bytes(sizeof(int) * lists);
        }
      })))
    return rc;
  A.idx_out = *pool_idx; A.score_out = *pool_score;
  c->plan.valid = 1; c->plan.diverse_path = split; c->plan.diverse_splits = split ? A.n_split : 0; c->plan.diverse_split_max = c->diverse_split_max;
  HIPCHK(c, poi::launch_diverse_pool(A, st, &c->tm));
  return POI_OK;
}

static int diverse_rerank_run(poi_ctx* c, const int32_t* pool_idx, const float* pool_score, int32_t n, int32_t pool, const void* items,
                              int32_t n_item, int32_t dim, const double* coords, const double* cphi, int32_t k, double trade,
                              double geo_weight, double scale_km, int32_t* idx_out, float* score_out, int32_t* pos_out, double* obj_out,
                              hipStream_t st) {
  poi::RerankArgs R = {};
  R.pool_idx = pool_idx; R.pool_score = pool_score; R.n = n; R.pool = pool;
  R.n_item = n_item; R.k = k; R.trade = trade; R.geo_weight = geo_weight; R.scale_km = scale_km;
  if (geo_weight < 1.0) { R.items = items; R.items_f16 = is_f16(c, items); R.dim = dim; }
  if (geo_weight > 0.0) { R.coords = coords; R.cphi = cphi; }
  R.idx_out = idx_out; R.score_out = score_out; R.pos_out = pos_out; R.obj_out = obj_out;
  if (int rc = bad_counter(c, st, &R.bad)) return rc;
  HIPCHK(c, poi::launch_diverse_rerank(R, st, &c->tm));
  return POI_OK;
}

int poi_diverse_pool(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                     const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                     const int32_t* ex_off, const int32_t* ex, int32_t pool, int32_t* pool_idx, float* pool_score, int32_t* count_out,
                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if (int rc = diverse_pool_check(c, "poi_diverse_pool", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex,
                                  pool, st, &T))
    return rc;
  if (!pool_idx || !pool_score) return fail(c, POI_EINVAL, "poi_diverse_pool: NULL pool_idx / pool_score");
  if (n == 0) return POI_OK;
  return diverse_pool_run(c, T, pool, &pool_idx, &pool_score, count_out, st);
}

int poi_diverse_rerank(poi_ctx* c, const int32_t* pool_idx, const float* pool_score, int32_t n, int32_t pool, const float* items, int32_t n_item,
                       int32_t dim, const double* coords, const double* cphi, int32_t k, double trade, double geo_weight, double scale_km,
                       int32_t* idx_out, float* score_out, int32_t* pos_out, double* obj_out, void* stream) {
  if (int rc = diverse_rerank_check(c, "poi_diverse_rerank", n, pool, items, n_item, dim, coords, cphi, k, trade, geo_weight, scale_km, idx_out))
    return rc;
  if (!pool_idx || !pool_score) return fail(c, POI_EINVAL, "poi_diverse_rerank: NULL pool_idx / pool_score");
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  return diverse_rerank_run(c, pool_idx, pool_score, n, pool, items, n_item, dim, coords, cphi, k, trade, geo_weight, scale_km, idx_out, score_out,
                            pos_out, obj_out, st);
}

int poi_diverse_topk(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                     const double* coords, const double* cphi, const double* thr, const int32_t* last_poi, int32_t n_dist, double dd,
                     const int32_t* ex_off, const int32_t* ex, int32_t pool, int32_t k, double trade, double geo_weight, double scale_km,
                     int32_t* idx_out, float* score_out, int32_t* pos_out, double* obj_out, int32_t* pool_idx, float* pool_score,
                     int32_t* count_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  int rc;
  if ((rc = diverse_pool_check(c, "poi_diverse_topk", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, last_poi, n_dist, dd, ex_off, ex, pool,
                               st, &T)))
    return rc;
  if ((rc = diverse_rerank_check(c, "poi_diverse_topk", n, pool, items, n_item, dim, coords, cphi, k, trade, geo_weight, scale_km, idx_out))) return rc;
  if ((pool_idx == nullptr) != (pool_score == nullptr)) return fail(c, POI_EINVAL, "poi_diverse_topk: pool_idx and pool_score go together");
  if (n == 0) return POI_OK;
  if ((rc = diverse_pool_run(c, T, pool, &pool_idx, &pool_score, count_out, st))) return rc;
  return diverse_rerank_run(c, pool_idx, pool_score, n, pool, items, n_item, dim, coords, cphi, k, trade, geo_weight, scale_km, idx_out, score_out,
                            pos_out, obj_out, st);
}

// ---------------------------------------------------------------------------------------------
// filtered recommendation (filter.hip)
int poi_filter_build(poi_ctx* c, const int32_t* cat, const uint32_t* flags, int32_t n_item, int32_t n_cat, const int32_t* pc_off, const int32_t* pc,
                     const uint32_t* need, const uint32_t* any, const uint32_t* forbid, int32_t n_pred, uint32_t* bits_out, int64_t ldw,
                     int32_t* count_out, void* stream) {
  if (!c) return fail(c, POI_EINVAL, "poi_filter_build: NULL ctx");
  if (n_item <= 0 || n_pred < 0) return fail(c, POI_EINVAL, "poi_filter_build: n_item <= 0 or P < 0");
  if (n_cat < 1 || n_cat > FILTER_NCAT_MAX) return fail(c, POI_EINVAL, "poi_filter_build: n_cat must lie in [1, %d] (got %d)", FILTER_NCAT_MAX, n_cat);
  if (ldw < ((int64_t)n_item + 31) / 32) return fail(c, POI_EINVAL, "poi_filter_build: ldw must be >= ceil(n_item / 32) = %d (got %lld)", (n_item + 31) / 32, (long long)ldw);
  if (n_pred == 0) return POI_OK;
  if (!pc_off || !need || !any || !forbid || !bits_out) return fail(c, POI_EINVAL, "poi_filter_build: NULL pc_off / need / any / forbid / bits_out");
  if (n_pred > 65535) return fail(c, POI_ENOTSUP, "poi_filter_build supports at most 65535 predicates per call (got %d)", n_pred);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  if (!cat || !pc) {      // a category list needs both: the offsets are the caller's device array, one look at the last one settles it
    int32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, pc_off + n_pred, sizeof(total), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (total > 0) return fail(c, POI_EINVAL, "poi_filter_build: a predicate with a category list needs cat and pc");
  }
  poi::FilterBuildArgs A = {};
  A.cat = cat; A.flags = flags; A.n_item = n_item; A.n_cat = n_cat;
  A.pc_off = pc_off; A.pc = pc; A.need = need; A.any = any; A.forbid = forbid; A.n_pred = n_pred;
  A.bits = bits_out; A.ldw = ldw; A.count = count_out;
  if (int rc = bad_counter(c, st, &A.bad)) return rc;
  // The kernel's workgroups read the predicate words while others already write bits_out: a caller whose bits_out overlaps need /
  // any / forbid (one scratch array handed for all of them) would have a late workgroup see a written word as its flag condition and read flags[j] for every POI - beyond a flags array that the all-zero words promised nobody would
  // read.  The words are copied aside first; the stream orders the copies before the kernel.
  uint32_t* words = nullptr;
  if (int rc = carve(c, c->filter_ws, st, [&](Carver& W) { words = (uint32_t*)W.bytes(sizeof(uint32_t) * 3 * (size_t)n_pred); })) return rc;
  const uint32_t* const src[3] = {need, any, forbid};
  for (int i = 0; i < 3; ++i) HIPCHK(c, hipMemcpyAsync(words + (size_t)i * n_pred, src[i], sizeof(uint32_t) * (size_t)n_pred, hipMemcpyDeviceToDevice, st));
  A.need = words; A.any = words + n_pred; A.forbid = words + 2 * (size_t)n_pred;
  HIPCHK(c, poi::launch_filter_build(A, st, &c->tm));
  return POI_OK;
}

// what the two ranking entries check alike: k, the bitmap and the per-row predicate index
static int filter_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const uint32_t* bits, int64_t ldw, int32_t n_pred, int32_t k,
                        const int32_t* idx_out) {
  if (!bits || !idx_out) return fail(c, POI_EINVAL, "%s: NULL bits / idx_out", who);
  if (k <= 0 || k > FILTER_K_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, FILTER_K_MAX, k);
  if (n < 0 || n_item <= 0 || n_pred <= 0) return fail(c, POI_EINVAL, "%s: n < 0, n_item <= 0 or n_pred <= 0", who);
  if (ldw < ((int64_t)n_item + 31) / 32) return fail(c, POI_EINVAL, "%s: ldw must be >= ceil(n_item / 32) = %d (got %lld)", who, (n_item + 31) / 32, (long long)ldw);
  return POI_OK;
}

int poi_score_topk_filtered(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                            const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor, int32_t n_dist,
                            double dd, const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred, int64_t cand_hint,
                            const int32_t* lat_order, double c_r, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t path,
                            int32_t* idx_out, float* score_out, int32_t* count_out, void* stream) {
  const char* who = "poi_score_topk_filtered";
  if (!c || !users || !items) return fail(c, POI_EINVAL, "%s: NULL ctx / users / items", who);
  int rc;
  if ((rc = filter_check(c, who, n, n_item, bits, ldw, n_pred, k, idx_out))) return rc;
  if (path != POI_FILTER_AUTO && path != POI_FILTER_WALK && path != POI_FILTER_GATHER) return fail(c, POI_EINVAL, "%s: unknown path %d", who, path);
  if (!(c_r >= 0.0)) return fail(c, POI_EINVAL, "%s: c_r must be >= 0 (+inf: no radius test)", who);
  if (cand_hint < 0) return fail(c, POI_EINVAL, "%s: cand_hint must be >= 0 (0: unknown)", who);
  const bool radius = c_r < HUGE_VAL;
  if (radius && path == POI_FILTER_WALK) return fail(c, POI_ENOTSUP, "%s: the walk path takes no radius", who);
  if (radius && (!coords || !cphi || !anchor || !lat_order)) return fail(c, POI_EINVAL, "%s: a radius needs coords / cphi / anchor / lat_order", who);
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if ((rc = tile_operands(c, who, users, items, n, n_item, dim, wd, sts, coords, cphi, thr, anchor, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (wd && n_dist > FILTER_NDIST_MAX) return fail(c, POI_ENOTSUP, "%s supports n_dist <= %d (got %d)", who, FILTER_NDIST_MAX, n_dist);
  if (n == 0) return POI_OK;
  poi::FilterArgs A = {};
  put_operands(A, T);
  A.last_poi = anchor; A.coords = coords; A.cphi = cphi;      // (the anchor is range-checked with or without a distance term)
  A.k = k; A.bits = bits; A.ldw = ldw; A.n_pred = n_pred; A.pred = pred;
  A.order = lat_order; A.c_r = c_r; A.band_deg = radius ? lat_band_deg(c_r) : 0.0;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  const int way = plan_filter_path(path, radius, n, n_item, cand_hint, c->filter_gather_cost);
  // few rows (live traffic): the item range of every 32-row tile (walk) / every row's candidates (gather) are cut into slices so that
  // the call fills the CUs; many rows: one workgroup per tile / row
  const int n_utile = (n + 31) / 32, ntile = (n_item + 31) / 32;
  const SplitPlan sp = way == FILTER_PATH_WALK
                           ? plan_split(n, n_utile, c->filter_split_max, c->filter_grid, 2, c->num_cu, ntile / 16, 2, FILTER_SPLIT_LIMIT)
                           : plan_split(n, n, c->filter_split_max, c->filter_grid, 4, c->num_cu, INT_MAX, 2, FILTER_SPLIT_LIMIT);
  A.n_split = sp.n_split;
  if (sp.split && (rc = carve_lists(c, c->filter_ws, st, A, (size_t)n * A.n_split, FILTER_K_MAX))) return rc;
  c->plan.valid = 1; c->plan.filter_path = way; c->plan.filter_splits = sp.split ? A.n_split : 0; c->plan.filter_split_max = c->filter_split_max;
  HIPCHK(c, way == FILTER_PATH_WALK ? poi::launch_filter_walk(A, st, &c->tm) : poi::launch_filter_gather(A, st, &c->tm));
  return POI_OK;
}

int poi_topk_filtered_scores(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, int64_t ld, const uint32_t* bits, int64_t ldw,
                             int32_t n_pred, const int32_t* pred, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out,
                             float* score_out, int32_t* count_out, void* stream) {
  const char* who = "poi_topk_filtered_scores";
  if (!c || !scores) return fail(c, POI_EINVAL, "%s: NULL ctx / scores", who);
  int rc;
  if ((rc = filter_check(c, who, n, n_item, bits, ldw, n_pred, k, idx_out))) return rc;
  if (ld < n_item) return fail(c, POI_EINVAL, "%s: ld must be >= n_item", who);
  if ((rc = check_ex_pair(c, who, ex_off, ex))) return rc;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::FilterScoresArgs A = {};
  A.scores = scores; A.ld = ld; A.n = n; A.n_item = n_item; A.k = k;
  A.ex_off = ex_off; A.ex = ex; A.bits = bits; A.ldw = ldw; A.n_pred = n_pred; A.pred = pred; A.n_split = 1;
  A.idx_out = idx_out; A.score_out = score_out; A.count_out = count_out;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  HIPCHK(c, poi::launch_filter_scores(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// capped recommendation (capped.hip)
int poi_labels_build(poi_ctx* c, const int32_t* labels, int32_t n_item, int32_t n_label, const uint32_t* bits, int64_t ldw, int32_t n_pred,
                     int32_t* count_out, int32_t* fill_out, void* stream) {
  const char* who = "poi_labels_build";
  if (!c || !labels || !fill_out) return fail(c, POI_EINVAL, "%s: NULL ctx / labels / fill_out", who);
  if (n_item <= 0 || n_label < 1 || n_label > n_item) return fail(c, POI_EINVAL, "%s: needs n_item > 0 and 1 <= n_label <= n_item (got %d, %d)", who, n_item, n_label);
  if (bits ? n_pred <= 0 : n_pred != 0) return fail(c, POI_EINVAL, "%s: n_pred must be > 0 with bits and 0 without (got %d)", who, n_pred);
  if (bits && ldw < ((int64_t)n_item + 31) / 32) return fail(c, POI_EINVAL, "%s: ldw must be >= ceil(n_item / 32) = %d (got %lld)", who, (n_item + 31) / 32, (long long)ldw);
  if (n_pred > 65535) return fail(c, POI_ENOTSUP, "%s supports at most 65535 predicates per call (got %d)", who, n_pred);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::LabelsBuildArgs A = {};
  A.labels = labels; A.n_item = n_item; A.n_label = n_label; A.bits = bits; A.ldw = ldw; A.n_pred = n_pred;
  const size_t rows = n_pred > 0 ? n_pred : 1;
  // the histogram is (predicates, n_label + 1) ints: many predicates over thousands of labels go through it "capped_hist_kb" KiB at a
  // time, the stream ordering one chunk's kernels before the next chunk's memset
  const size_t per_row = sizeof(int) * ((size_t)n_label + 1);
  size_t chunk = ((size_t)c->capped_hist_kb << 10) / per_row;
  chunk = chunk < 1 ? 1 : (chunk > rows ? rows : chunk);
  int rc;
  if ((rc = carve(c, c->capped_ws, st, [&](Carver& W) { A.hist = (int*)W.bytes(per_row * chunk); }))) return rc;
  int* bad = nullptr;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  for (size_t q0 = 0; q0 < rows; q0 += chunk) {
    const size_t m = rows - q0 < chunk ? rows - q0 : chunk;
    A.bits = bits ? bits + q0 * (size_t)ldw : nullptr;
    A.n_pred = bits ? (int)m : 0;
    A.unl = A.hist + m * n_label;
    A.fill = fill_out + q0 * CAPPED_FILL_LD;
    A.count = q0 == 0 ? count_out : nullptr;             // the per-label counts and the stray labels do not depend on the predicate:
    A.bad = q0 == 0 ? bad : nullptr;                     // the first chunk reports them
    HIPCHK(c, poi::launch_labels_build(A, st, &c->tm));
  }
  return POI_OK;
}

// what the two ranking entries check alike: k, the cap, the labels, the optional bitmap
static int capped_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* labels, int32_t per, const uint32_t* bits,
                        int64_t ldw, int32_t n_pred, int32_t k, const int32_t* idx_out) {
  if (k <= 0 || k > CAPPED_K_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= k <= %d (got %d)", who, CAPPED_K_MAX, k);
  if (per <= 0 || per > CAPPED_PER_MAX) return fail(c, POI_ENOTSUP, "%s supports 1 <= per <= %d (got %d)", who, CAPPED_PER_MAX, per);
  if (!labels || !idx_out) return fail(c, POI_EINVAL, "%s: NULL labels / idx_out", who);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if (bits && n_pred <= 0) return fail(c, POI_EINVAL, "%s: n_pred must be > 0 with bits", who);
  if (bits && ldw < ((int64_t)n_item + 31) / 32) return fail(c, POI_EINVAL, "%s: ldw must be >= ceil(n_item / 32) = %d (got %lld)", who, (n_item + 31) / 32, (long long)ldw);
  return POI_OK;
}

int poi_score_topk_capped(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                          const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor, int32_t n_dist,
                          double dd, const int32_t* labels, int32_t per, const int32_t* fill, const uint32_t* bits, int64_t ldw, int32_t n_pred,
                          const int32_t* pred, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out,
                          int32_t* label_out, int32_t* count_out, void* stream) {
  const char* who = "poi_score_topk_capped";
  if (!c || !users || !items) return fail(c, POI_EINVAL, "%s: NULL ctx / users / items", who);
  int rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, dim);
  if ((rc = capped_check(c, who, n, n_item, labels, per, bits, ldw, n_pred, k, idx_out))) return rc;
  if ((rc = tile_operands(c, who, users, items, n, n_item, dim, wd, sts, coords, cphi, thr, anchor, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (wd && n_dist > CAPPED_NDIST_MAX) return fail(c, POI_ENOTSUP, "%s supports n_dist <= %d (got %d)", who, CAPPED_NDIST_MAX, n_dist);
  if (n == 0) return POI_OK;
  poi::CappedArgs A = {};
  put_operands(A, T);
  A.last_poi = anchor; A.coords = coords; A.cphi = cphi;      // (the anchor is range-checked with or without a distance term)
  A.k = k; A.labels = labels; A.per = per; A.fill = fill;
  A.bits = bits; A.ldw = bits ? ldw : 0; A.n_pred = bits ? n_pred : 1; A.pred = bits ? pred : nullptr;
  A.idx_out = idx_out; A.score_out = score_out; A.label_out = label_out; A.count_out = count_out;
  // few rows (live traffic): the item range of every 32-row tile is cut into slices so that the call fills the CUs; many rows: one
  // workgroup per tile
  const int n_utile = (n + 31) / 32, ntile = (n_item + 31) / 32;
  const SplitPlan sp = plan_split(n, n_utile, c->capped_split_max, c->capped_grid, 2, c->num_cu, ntile / 16, 2, CAPPED_SPLIT_LIMIT);
  A.n_split = sp.n_split;
  if (sp.split && (rc = carve_lists(c, c->capped_ws, st, A, (size_t)n * A.n_split, CAPPED_K_MAX))) return rc;
  c->plan.valid = 1; c->plan.capped_splits = sp.split ? A.n_split : 0; c->plan.capped_split_max = c->capped_split_max;
  HIPCHK(c, poi::launch_capped_walk(A, st, &c->tm));
  return POI_OK;
}

int poi_topk_capped_scores(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, int64_t ld, const int32_t* labels, int32_t per,
                           const int32_t* fill, const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred, const int32_t* ex_off,
                           const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out, int32_t* label_out, int32_t* count_out,
                           void* stream) {
  const char* who = "poi_topk_capped_scores";
  if (!c || !scores) return fail(c, POI_EINVAL, "%s: NULL ctx / scores", who);
  int rc;
  if ((rc = capped_check(c, who, n, n_item, labels, per, bits, ldw, n_pred, k, idx_out))) return rc;
  if (ld < n_item) return fail(c, POI_EINVAL, "%s: ld must be >= n_item", who);
  if ((rc = check_ex_pair(c, who, ex_off, ex))) return rc;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::CappedScoresArgs A = {};
  A.scores = scores; A.ld = ld; A.n = n; A.n_item = n_item; A.k = k;
  A.ex_off = ex_off; A.ex = ex; A.labels = labels; A.per = per; A.fill = fill;
  A.bits = bits; A.ldw = bits ? ldw : 0; A.n_pred = bits ? n_pred : 1; A.pred = bits ? pred : nullptr;
  A.idx_out = idx_out; A.score_out = score_out; A.label_out = label_out; A.count_out = count_out;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  HIPCHK(c, poi::launch_capped_scores(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// label recommendation (labels.hip)
struct LabelsOut {      // what a call asks of the finish kernel: pointers at row 0
  uint64_t* mass; int32_t* best_id; float* best_score; int32_t* count;      // dense (n, n_label + 1)
  float* m; double* lognorm;                                                // (n)
  int32_t* label; double* logp; int32_t* top_id; float* top_score;          // (n, k)
  int32_t* n_listed; double* rest_logp;                                     // (n)
};

// what the three entries check alike
static int labels_check(poi_ctx* c, const char* who, int32_t n, int32_t n_item, const int32_t* labels, int32_t n_label, int32_t by, int32_t k,
                        bool topk_required, const int32_t* label_out) {
  if (k > LABELS_K_MAX || k < (topk_required ? 1 : 0))
    return fail(c, POI_ENOTSUP, "%s supports %d <= k <= %d (got %d)", who, topk_required ? 1 : 0, LABELS_K_MAX, k);
  if (!labels) return fail(c, POI_EINVAL, "%s: NULL labels", who);
  if (k > 0 && !label_out) return fail(c, POI_EINVAL, "%s: NULL label_out", who);
  if (k > 0 && by != LABELS_BY_MASS && by != LABELS_BY_MAX) return fail(c, POI_EINVAL, "%s: by must be POI_LABELS_BY_MASS or POI_LABELS_BY_MAX (got %d)", who, by);
  if (n < 0 || n_item <= 0) return fail(c, POI_EINVAL, "%s: n < 0 or n_item <= 0", who);
  if (n_item >= (1 << 27)) return fail(c, POI_ENOTSUP, "%s supports n_item < 2^27: the 64-bit mass of a label must stay below 2^63 (got %d)", who, n_item);
  if (n_label < 1 || n_label > n_item) return fail(c, POI_EINVAL, "%s: needs 1 <= n_label <= n_item (got %d, %d)", who, n_label, n_item);
  return POI_OK;
}

// The rows of a call through the accumulator workspace, "labels_ws_kb" KiB of whole 32-row tiles at a time: per chunk the memset, the
// accumulation (`accumulate(row0, rows, acc)`: the max pass and the walk, or the explicit-rows kernel) and the finish kernel.
static int labels_run(poi_ctx* c, int n, int n_label, int by, int k, const LabelsOut& O, hipStream_t st,
                      const std::function<int(int, int, const poi::LabelsAcc&)>& accumulate) {
  const size_t L1 = (size_t)n_label + 1, per_row = LABELS_ROW_BYTES * L1 + 8;
  size_t fit = ((size_t)c->labels_ws_kb << 10) / per_row / 32 * 32;
  if (fit < 32) fit = 32;
  const size_t n_pad = ((size_t)n + 31) / 32 * 32;
  const size_t chunk = fit < n_pad ? fit : n_pad;
  poi::LabelsAcc acc = {};
  void* block = nullptr;
  const size_t bytes = chunk * per_row;
  int rc;
  if ((rc = carve(c, c->labels_ws, st, [&](Carver& W) { block = W.bytes(bytes); }))) return rc;
  acc.mass = (unsigned long long*)block; acc.best = acc.mass + chunk * L1; acc.cnt = (unsigned*)(acc.best + chunk * L1);
  acc.mkey = acc.cnt + chunk * L1; acc.status = (int*)(acc.mkey + chunk);
  c->plan.valid = 1; c->plan.labels_rows_per_chunk = (int)chunk; c->plan.labels_chunks = (int)((n_pad + chunk - 1) / chunk);
  for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk) {
    const int m = (int)((size_t)n - r0 < chunk ? (size_t)n - r0 : chunk);
    HIPCHK(c, hipMemsetAsync(block, 0, bytes, st));      // (the stream orders it behind the finish kernel of the chunk before)
    if ((rc = accumulate((int)r0, m, acc))) return rc;
    poi::LabelsFinishArgs F = {};
    F.n = m; F.n_label = n_label; F.k = k; F.by = by; F.acc = acc;
    F.mass_out = O.mass ? (unsigned long long*)O.mass + r0 * L1 : nullptr; F.best_id_out = O.best_id ? O.best_id + r0 * L1 : nullptr;
    F.best_score_out = O.best_score ? O.best_score + r0 * L1 : nullptr; F.count_out = O.count ? O.count + r0 * L1 : nullptr;
    F.m_out = O.m ? O.m + r0 : nullptr; F.lognorm_out = O.lognorm ? O.lognorm + r0 : nullptr;
    F.label_out = O.label ? O.label + r0 * k : nullptr; F.logp_out = O.logp ? O.logp + r0 * k : nullptr;
    F.top_id_out = O.top_id ? O.top_id + r0 * k : nullptr; F.top_score_out = O.top_score ? O.top_score + r0 * k : nullptr;
    F.n_listed_out = O.n_listed ? O.n_listed + r0 : nullptr; F.rest_logp_out = O.rest_logp ? O.rest_logp + r0 : nullptr;
    HIPCHK(c, poi::launch_labels_finish(F, st, &c->tm));
  }
  return POI_OK;
}

// the fused entries: the tile walk over users . items
static int labels_fused(poi_ctx* c, const char* who, const char* span_name, const float* users, const float* items, int32_t n, int32_t n_item,
                        int32_t dim, const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr,
                        const int32_t* anchor, int32_t n_dist, double dd, const int32_t* labels, int32_t n_label, const int32_t* ex_off,
                        const int32_t* ex, int32_t by, int32_t k, bool topk_required, const LabelsOut& O, void* stream) {
  if (!c || !users || !items) return fail(c, POI_EINVAL, "%s: NULL ctx / users / items", who);
  int rc;
  hipStream_t st = (hipStream_t)stream;
  poi::TileOperands T;
  if (dim <= 0 || dim % 4 != 0 || dim > 256) return fail(c, POI_ENOTSUP, "%s: dim must be a multiple of 4 in [4, 256] (got %d)", who, dim);
  if ((rc = labels_check(c, who, n, n_item, labels, n_label, by, k, topk_required, O.label))) return rc;
  if ((rc = tile_operands(c, who, users, items, n, n_item, dim, wd, sts, coords, cphi, thr, anchor, n_dist, dd, ex_off, ex, st, &T))) return rc;
  if (wd && n_dist > LABELS_NDIST_MAX) return fail(c, POI_ENOTSUP, "%s supports n_dist <= %d (got %d)", who, LABELS_NDIST_MAX, n_dist);
  if (n == 0) return POI_OK;
  const bool lds_home = poi::labels_lds_bytes(32, n_label) <= ((size_t)c->labels_lds_kb << 10);
  const int ntile = (n_item + 31) / 32;
  c->plan.labels_home = lds_home ? 1 : 2; c->plan.labels_split_max = c->labels_split_max;
  const long span = c->tm.span_begin(span_name, st);      // the call; inside it the max pass, the walk and the finish on their own
  rc = labels_run(c, n, n_label, by, k, O, st, [&](int r0, int m, const poi::LabelsAcc& acc) -> int {
    poi::LabelsArgs A = {};
    put_operands(A, T);
    A.users = users + (size_t)r0 * dim; A.n = m;
    A.last_poi = anchor ? anchor + r0 : nullptr; A.coords = coords; A.cphi = cphi;      // (the anchor is range-checked with or without a distance term)
    if (A.sts) A.sts = sts + (size_t)r0 * ((size_t)n_dist + 1);
    if (A.ex_off) A.ex_off = ex_off + r0;
    A.labels = labels; A.n_label = n_label; A.lds_home = lds_home; A.acc = acc;
    // few rows (live traffic): the item range of every 32-row tile is cut into slices so that the call fills the CUs; many rows: one
    // workgroup per tile
    const SplitPlan sp = plan_split(m, (m + 31) / 32, c->labels_split_max, c->labels_grid, 2, c->num_cu, ntile / 16, 2, LABELS_SPLIT_LIMIT);
    A.n_split = sp.n_split;
    c->plan.labels_splits = sp.split ? A.n_split : 0;
    HIPCHK(c, poi::launch_labels_max(A, st, &c->tm));
    HIPCHK(c, poi::launch_labels_walk(A, st, &c->tm));
    return POI_OK;
  });
  c->tm.span_end(span, st);
  return rc;
}

int poi_score_labels(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd, const float* sts,
                     const double* coords, const double* cphi, const double* thr, const int32_t* anchor, int32_t n_dist, double dd,
                     const int32_t* labels, int32_t n_label, const int32_t* ex_off, const int32_t* ex, uint64_t* mass_out, int32_t* best_id_out,
                     float* best_score_out, int32_t* count_out, float* m_out, double* lognorm_out, void* stream) {
  LabelsOut O = {};
  O.mass = mass_out; O.best_id = best_id_out; O.best_score = best_score_out; O.count = count_out; O.m = m_out; O.lognorm = lognorm_out;
  return labels_fused(c, "poi_score_labels", "score_labels", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, anchor, n_dist, dd, labels,
                      n_label, ex_off, ex, LABELS_BY_MASS, 0, false, O, stream);
}

int poi_score_topk_labels(poi_ctx* c, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                          const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor, int32_t n_dist,
                          double dd, const int32_t* labels, int32_t n_label, const int32_t* ex_off, const int32_t* ex, int32_t by, int32_t k,
                          int32_t* label_out, double* logp_out, int32_t* best_id_out, float* best_score_out, int32_t* n_listed_out,
                          double* rest_logp_out, float* m_out, double* lognorm_out, void* stream) {
  LabelsOut O = {};
  O.label = label_out; O.logp = logp_out; O.top_id = best_id_out; O.top_score = best_score_out; O.n_listed = n_listed_out;
  O.rest_logp = rest_logp_out; O.m = m_out; O.lognorm = lognorm_out;
  return labels_fused(c, "poi_score_topk_labels", "score_topk_labels", users, items, n, n_item, dim, wd, sts, coords, cphi, thr, anchor, n_dist, dd,
                      labels, n_label, ex_off, ex, by, k, true, O, stream);
}

int poi_labels_scores(poi_ctx* c, const float* scores, int32_t n, int32_t n_item, int64_t ld, const int32_t* labels, int32_t n_label,
                      const int32_t* ex_off, const int32_t* ex, int32_t by, int32_t k, uint64_t* mass_out, int32_t* best_id_out,
                      float* best_score_out, int32_t* count_out, int32_t* label_out, double* logp_out, int32_t* top_id_out, float* top_score_out,
                      int32_t* n_listed_out, double* rest_logp_out, float* m_out, double* lognorm_out, void* stream) {
  const char* who = "poi_labels_scores";
  if (!c || !scores) return fail(c, POI_EINVAL, "%s: NULL ctx / scores", who);
  int rc;
  if ((rc = labels_check(c, who, n, n_item, labels, n_label, by, k, false, label_out))) return rc;
  if (ld < n_item) return fail(c, POI_EINVAL, "%s: ld must be >= n_item", who);
  if ((rc = check_ex_pair(c, who, ex_off, ex))) return rc;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  int* bad = nullptr;
  if ((rc = bad_counter(c, st, &bad))) return rc;
  LabelsOut O = {};
  O.mass = mass_out; O.best_id = best_id_out; O.best_score = best_score_out; O.count = count_out; O.m = m_out; O.lognorm = lognorm_out;
  O.label = label_out; O.logp = logp_out; O.top_id = top_id_out; O.top_score = top_score_out; O.n_listed = n_listed_out; O.rest_logp = rest_logp_out;
  // one row per workgroup: its accumulators take 1 / 32 of a tile's - the same budget holds 32 times the labels
  const bool lds_home = poi::labels_lds_bytes(1, n_label) <= ((size_t)c->labels_lds_kb << 10);
  c->plan.labels_home = lds_home ? 1 : 2; c->plan.labels_splits = 0; c->plan.labels_split_max = c->labels_split_max;
  const long span = c->tm.span_begin("labels_scores_call", st);
  rc = labels_run(c, n, n_label, by, k, O, st, [&](int r0, int m, const poi::LabelsAcc& acc) -> int {
    poi::LabelsScoresArgs A = {};
    A.scores = scores + (size_t)r0 * (size_t)ld; A.ld = ld; A.n = m; A.n_item = n_item;
    A.ex_off = ex_off ? ex_off + r0 : nullptr; A.ex = ex; A.labels = labels; A.n_label = n_label; A.lds_home = lds_home; A.acc = acc; A.bad = bad;
    HIPCHK(c, poi::launch_labels_scores(A, st, &c->tm));
    return POI_OK;
  });
  c->tm.span_end(span, st);
  return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  A.dummy = (const double*)(A.bad + 8);      // (bytes 32 .. 39 of the counter's buffer: never written)
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

}  // extern "C"
