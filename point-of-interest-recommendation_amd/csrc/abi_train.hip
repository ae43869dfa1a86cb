// C-ABI of libpoi_hip.so (see include/poi_hip.h): the training steps of the models besides the GRU family - BPR-MF, VBPR, FPMC-LR, PRME, GeoIE, POI2Vec, Lstm / Rnn.
#include "abi_internal.h"

#include <string.h>

// parameter checks shared with the scoring entries of abi_serve.hip
int prme_check(poi_ctx* c, const poi_prme_params* P, const char* who) {
  if (!c || !P || !P->du || !P->dp || !P->ds) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->du) || is_f16(c, P->dp) || is_f16(c, P->ds)) return fail(c, POI_ENOTSUP, "PRME tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "PRME: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "%s: bad sizes", who);
  return POI_OK;
}

int geoie_check(poi_ctx* c, const poi_geoie_params* P, const char* who) {
  if (!c || !P || !P->g || !P->h || !P->t || !P->z || !P->ab) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->g) || is_f16(c, P->h) || is_f16(c, P->t) || is_f16(c, P->z)) return fail(c, POI_ENOTSUP, "GeoIE tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "GeoIE: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->n_user <= 0 || P->n_item <= 0) return fail(c, POI_EINVAL, "%s: bad sizes", who);
  return POI_OK;
}

int poi2vec_check(poi_ctx* c, const poi_poi2vec_params* P, const char* who) {
  if (!c || !P || !P->xu || !P->wl || !P->pb || !P->routes || !P->lrs || !P->probs || !P->rid) return fail(c, POI_EINVAL, "%s: NULL argument", who);
  if (is_f16(c, P->xu) || is_f16(c, P->wl) || is_f16(c, P->pb)) return fail(c, POI_ENOTSUP, "POI2Vec tables are float32 only");
  if (P->dim <= 0 || P->dim % 4 != 0 || P->dim > 128) return fail(c, POI_ENOTSUP, "POI2Vec: dim must be a multiple of 4 in [4, 128] (got %d)", P->dim);
  if (P->depth < 1 || P->depth > 31) return fail(c, POI_ENOTSUP, "POI2Vec: depth must lie in [1, 31] (got %d)", P->depth);
  if (P->n_user <= 0 || P->n_item <= 0 || (int64_t)P->n_node != ((int64_t)1 << P->depth) - 1)
    return fail(c, POI_EINVAL, "%s: bad sizes (n_node must be 2^depth - 1)", who);
  return POI_OK;
}

extern "C" {

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
  if (int r = refuse_batch_cap0(c)) return r;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::BprArgs A;
  memset(&A, 0, sizeof A);
  A.ux = ux; A.lt = lt; A.n_user = n_user; A.n_item = n_item; A.dim = dim;
  A.lt_f16 = is_f16(c, lt);
  A.sr_salt = (c->f16_rounding && A.lt_f16) ? (++c->sr_counter) * 0x9E3779B1u | 1u : 0u;
  A.uidx = uidx; A.p = p; A.q = q; A.n = n; A.alpha = alpha; A.lambda = lambda; A.loss = loss_out; A.bcap = c->batch_cap;
  if (int r = bad_counter(c, st, &A.bad)) return r;
  if (mode == POI_BPR_SNAPSHOT) {
    // workspace: the 3 n touches' sort buffers, per-triple coefficients, per-window partial sums; the shadow user table (grow-only, ctx-owned)
    int rc;
    if ((rc = ensure(c, c->g_ux, sizeof(float) * (size_t)n_user * dim, st))) return rc;
    A.shadow = (float*)c->g_ux.p;
    const size_t chunks = (size_t)(n + 63) / 64 + (size_t)(2 * (size_t)n + 63) / 64 + 2;
    if ((rc = carve(c, c->g_blt, st, [&](Carver& W) {
          carve_sort(A, W, 3, n, chunks);
          A.g = (float*)W.bytes(sizeof(float) * ((size_t)n + 64));
          A.lead = (float*)W.bytes(sizeof(float) * chunks * dim);      // (lead / trail rows are read as float4)
          A.trail = (float*)W.bytes(sizeof(float) * chunks * dim);
        }))) return rc;
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
  if (int r = refuse_batch_cap0(c)) return r;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  A.uidx = uidx; A.p = p; A.q = q; A.n = n; A.alpha = alpha; A.lambda = lambda; A.lambda_ev = lambda_ev; A.bcap = c->batch_cap; A.loss = loss_out;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  poi::vbpr_chunking(n, &A.ch_rows, &A.n_chunk);
  const size_t chunks = ((size_t)4 * n + 63) / 64 + 2, D = (size_t)P->dim;
  if ((rc = carve(c, c->vb_ws, st, [&](Carver& W) {
        A.dpart = (double*)W.bytes(sizeof(double) * (size_t)A.n_chunk * D * P->n_img);
        carve_sort(A, W, 4, n, chunks);
        A.okf = (int*)W.bytes(sizeof(int) * ((size_t)n + 64));
        A.ord = (int*)W.bytes(sizeof(int) * ((size_t)n + 64));
        A.g = (float*)W.bytes(sizeof(float) * ((size_t)n + 64));
        A.V = (float*)W.bytes(sizeof(float) * n * D);
        A.lead = (float*)W.bytes(sizeof(float) * chunks * D);
        A.trail = (float*)W.bytes(sizeof(float) * chunks * D);
        A.slot = (float*)W.bytes(sizeof(float) * 4 * n * D);
      }))) return rc;
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
  if (int r = refuse_batch_cap0(c)) return r;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::FpmcArgs A;
  memset(&A, 0, sizeof A);
  A.ui = P->ui; A.iu = P->iu; A.ia = P->ia; A.ai = P->ai; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim;
  A.u = u; A.a = a; A.i = i; A.j = j; A.n = n; A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.loss = loss_out;
  A.sentinel = P->n_user + 3 * (P->n_item + 1);
  int rc;
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  const size_t chunks = ((size_t)6 * n + 63) / 64 + 2, D = (size_t)P->dim;
  if ((rc = carve(c, c->fp_ws, st, [&](Carver& W) {
        carve_sort(A, W, 6, n, chunks);
        A.s = (float*)W.bytes(sizeof(float) * ((size_t)n + 64));
        A.lead = (float*)W.bytes(sizeof(float) * chunks * D);
        A.trail = (float*)W.bytes(sizeof(float) * chunks * D);
        A.slot = (float*)W.bytes(sizeof(float) * 6 * n * D);
      }))) return rc;
  HIPCHK(c, poi::launch_fpmc_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// PRME (prme.hip)
int poi_prme_step(poi_ctx* c, const poi_prme_params* P, const int32_t* u, const int32_t* p, const int32_t* q, const int32_t* prev,
                  const double* d, const int32_t* gap, int32_t n, float alpha, float lambda, int32_t threshold, float cw, float* loss_out,
                  void* stream) {
  int rc = prme_check(c, P, "poi_prme_step");
  if (rc) return rc;
  if (!u || !p || !q || !prev || !d || !gap || !loss_out) return fail(c, POI_EINVAL, "poi_prme_step: NULL argument");
  if (n < 0) return fail(c, POI_EINVAL, "poi_prme_step: bad sizes");
  if ((int64_t)P->n_user + 2 * ((int64_t)P->n_item + 1) >= ((int64_t)1 << 31) - 1) return fail(c, POI_ENOTSUP, "PRME: n_user + 2 (n_item + 1) must stay below 2^31");
  if ((int64_t)n * 7 >= ((int64_t)1 << 31) - 64) return fail(c, POI_ENOTSUP, "PRME: at most 2^31 / 7 transitions per launch");
  if (int r = refuse_batch_cap0(c)) return r;
  if (n == 0) return POI_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  poi::PrmeArgs A;
  memset(&A, 0, sizeof A);
  A.du = P->du; A.dp = P->dp; A.ds = P->ds; A.n_user = P->n_user; A.n_item = P->n_item; A.dim = P->dim;
  A.u = u; A.p = p; A.q = q; A.prev = prev; A.d = d; A.gap = gap; A.n = n; A.thd = threshold;
  A.alpha = alpha; A.lambda = lambda; A.bcap = c->batch_cap; A.cw = cw; A.loss = loss_out;
  A.sentinel = P->n_user + 2 * (P->n_item + 1);
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  const size_t chunks = ((size_t)7 * n + 63) / 64 + 2, D = (size_t)P->dim;
  if ((rc = carve(c, c->pr_ws, st, [&](Carver& W) {
        carve_sort(A, W, 7, n, chunks);
        A.ga = (float*)W.bytes(sizeof(float) * ((size_t)n + 64));
        A.gb = (float*)W.bytes(sizeof(float) * ((size_t)n + 64));
        A.lead = (float*)W.bytes(sizeof(float) * chunks * D);
        A.trail = (float*)W.bytes(sizeof(float) * chunks * D);
        A.slot = (float*)W.bytes(sizeof(float) * 7 * n * D);
      }))) return rc;
  HIPCHK(c, poi::launch_prme_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// GeoIE (geoie.hip)
// carve the GeoIE workspace for a launch of n users and P rows; pairs: also the pair offsets, and none of the step's gradient pieces
static int geoie_workspace(poi_ctx* c, poi::GeoieArgs& A, int n, int P, int dim, bool pairs, hipStream_t st) {
  const size_t N1 = (size_t)n + 1, P1 = (size_t)P + 1, chunks = pairs ? 0 : ((size_t)5 * P + 63) / 64 + 2, PD = pairs ? 0 : (size_t)P * dim;
  return carve(c, c->ge_ws, st, [&](Carver& W) {
    A.rowoff = (int*)W.bytes(sizeof(int) * N1); A.troff = (int*)W.bytes(sizeof(int) * N1); A.tcoff = (int*)W.bytes(sizeof(int) * N1);
    A.pairoff = pairs ? (long long*)W.bytes(sizeof(long long) * N1) : nullptr;
    A.ubad = (int*)W.bytes(sizeof(int) * N1); A.tot = (int*)W.bytes(sizeof(int) * 8);
    A.tuser = (int*)W.bytes(sizeof(int) * P1); A.coef = (float*)W.bytes(sizeof(float) * P1);
    A.rloss = (double*)W.bytes(sizeof(double) * P1 * 3); A.rda = A.rloss + P1; A.rdb = A.rda + P1;
    A.uda = (double*)W.bytes(sizeof(double) * N1 * 2); A.udb = A.uda + N1;
    A.G = (float*)W.bytes(sizeof(float) * 3 * PD);
    carve_sort(A, W, pairs ? 0 : 5, (size_t)P, 2 * chunks); A.meta2 = A.meta + chunks;
    A.lead = (float*)W.bytes(sizeof(float) * chunks * dim * 2); A.trail = A.lead + chunks * dim;
    A.slot = (float*)W.bytes(sizeof(float) * 5 * PD);
  });
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
  if (int r = refuse_batch_cap0(c)) return r;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  const size_t D = (size_t)P->dim, NO = (size_t)P->cell * D, Rp = R + 8, chunks = (E + 63) / 64 + 2, NW = sizeof(float4) * NO * (D / 4);
  if ((rc = carve(c, c->cell_ws, st, [&](Carver& W) {
        A.uiP = (float4*)W.bytes(NW); A.whP = (float4*)W.bytes(NW); A.uiT = (float4*)W.bytes(NW); A.whT = (float4*)W.bytes(NW);      // packed weights
        A.H = (double*)W.bytes(sizeof(double) * Rp * D); A.ACT = (double*)W.bytes(sizeof(double) * Rp * NO); A.CS = (double*)W.bytes(sizeof(double) * Rp * D);
        A.DX = (double*)W.bytes(sizeof(double) * Rp * D); A.gam = (double*)W.bytes(sizeof(double) * Rp);
        A.dpart = (double*)W.bytes(sizeof(double) * CELL_DENSE_CHUNKS * NO * (2 * D + 1));
        A.lead = (double*)W.bytes(sizeof(double) * chunks * D); A.trail = (double*)W.bytes(sizeof(double) * chunks * D);
        A.slot = (float*)W.bytes(sizeof(float) * (E + 64) * D);
        carve_sort(A, W, 1, E, chunks);
        A.rowp = (int*)W.bytes(sizeof(int) * Rp); A.slen = (int*)W.bytes(sizeof(int) * ((size_t)n + 8)); A.poff = (int*)W.bytes(sizeof(int) * ((size_t)n + 8));
        A.mm = (int*)W.bytes(sizeof(int) * chunks);
      }))) return rc;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  const size_t D = (size_t)P->dim, NO = (size_t)P->cell * D;
  if ((rc = ensure(c, c->cell_ws, 16 * 4 * NO * (D / 4) + 256, st))) return rc;
  float4* f4 = (float4*)c->cell_ws.p;
  A.uiP = f4; f4 += NO * (D / 4); A.whP = f4; f4 += NO * (D / 4); A.uiT = f4; f4 += NO * (D / 4); A.whT = f4;
  HIPCHK(c, poi::launch_cell_predict(A, st, &c->tm));
  return POI_OK;
}

// ---------------------------------------------------------------------------------------------
// POI2Vec (poi2vec.hip)
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
  if (int r = refuse_batch_cap0(c)) return r;
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
  if ((rc = bad_counter(c, st, &A.bad))) return rc;
  const int n_slot = A.n_tile < 256 ? A.n_tile : 256;
  if ((rc = carve(c, c->pv_ws, st, [&](Carver& W) {
        const size_t n = (size_t)A.n, P = (size_t)A.n_pos, R = 4 * (size_t)A.depth, D = (size_t)A.dim, E = P * R + 64, T = P + (size_t)A.n_ctx + 64;
        A.ubad = (int*)W.bytes(sizeof(int) * (n + 1)); A.acc = (int*)W.bytes(sizeof(int) * (n + 1)); A.lpos = (int*)W.bytes(sizeof(int) * (n + 1)); A.lctx = (int*)W.bytes(sizeof(int) * (n + 1));
        A.tot = (int*)W.bytes(sizeof(int) * (8)); A.cnt = (int*)W.bytes(sizeof(int) * (8));
        A.pmax = (float*)W.bytes(sizeof(float) * (n * A.n_tile + 1)); A.psum = (double*)W.bytes(sizeof(double) * (n * A.n_tile + 1));
        A.posval = (double*)W.bytes(sizeof(double) * (P + 1)); A.gz = (double*)W.bytes(sizeof(double) * (P * R + 1)); A.cbuf = (double*)W.bytes(sizeof(double) * (P * D + 1)); A.gcbuf = (double*)W.bytes(sizeof(double) * (P * D + 1));
        A.lse = (double*)W.bytes(sizeof(double) * (n + 1)); A.tsum = (double*)W.bytes(sizeof(double) * (n * D + 1)); A.scale = (float*)W.bytes(sizeof(float) * (8)); A.dxu = (float*)W.bytes(sizeof(float) * ((size_t)n_slot * n * D + 1));
        A.keys0 = (int*)W.bytes(sizeof(int) * (E)); A.keys1 = (int*)W.bytes(sizeof(int) * (E)); A.vals0 = (int*)W.bytes(sizeof(int) * (E)); A.vals1 = (int*)W.bytes(sizeof(int) * (E));
        A.k2a = (int*)W.bytes(sizeof(int) * (T)); A.k2b = (int*)W.bytes(sizeof(int) * (T)); A.v2a = (int*)W.bytes(sizeof(int) * (T)); A.v2b = (int*)W.bytes(sizeof(int) * (T)); A.epos = (int*)W.bytes(sizeof(int) * (T));
        A.hist = (int*)W.bytes(sizeof(int) * ((size_t)RS_HIST_INTS + RS_MAXBIN + 64));
      }))) return rc;
  HIPCHK(c, poi::launch_poi2vec_step(A, c->num_cu, st, &c->tm));
  return POI_OK;
}

}  // extern "C"
