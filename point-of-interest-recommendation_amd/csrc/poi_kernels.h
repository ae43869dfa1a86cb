// Internal (non-ABI) declarations shared between the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

struct ScorePlan;      // score_plan.h

namespace poi {

// Optional per-kernel timing with HIP events recorded on the launch stream (bench.py's live
// roofline measurement).  Disabled by default: begin()/end() are then no-ops.
struct Timing {
  struct Rec { std::string name; hipEvent_t a, b; };
  bool on = false;
  // sampling: with period N only every N-th training launch is instrumented (tick() at the launch's entry decides) - an event pair
  // per kernel costs ~7 us of stream serialisation, 7 % of a Gowalla epoch when every launch carries them; the average duration of
  // the sampled launches is the launch duration either way
  int period = 1; unsigned long count = 0; bool active = true;
  void tick() { active = period <= 1 || (count++ % (unsigned long)period) == 0; }
  std::vector<Rec> recs;
  size_t limit = 32768;
  void begin(const char* name, hipStream_t st) {
    if (!on || !active || recs.size() >= limit) { open_ = false; return; }
    Rec r; r.name = name;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) { open_ = false; return; }
    (void)hipEventRecord(r.a, st);
    recs.push_back(r); open_ = true;
  }
  void end(hipStream_t st) { if (open_) { (void)hipEventRecord(recs.back().b, st); open_ = false; } }
  // a region that spans other regions (a fork / join over two streams): closed through its index; -1 = not recorded
  long span_begin(const char* name, hipStream_t st) {
    if (!on || !active || recs.size() >= limit) return -1;
    Rec r; r.name = name;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return -1;
    (void)hipEventRecord(r.a, st);
    (void)hipEventRecord(r.b, st);          // (valid even if span_end is never reached)
    recs.push_back(r);
    return (long)recs.size() - 1;
  }
  void span_end(long idx, hipStream_t st) { if (idx >= 0 && (size_t)idx < recs.size()) (void)hipEventRecord(recs[(size_t)idx].b, st); }
  void clear() { for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } recs.clear(); }
  // a launcher's record: begun here, closed on every way out - close() on the normal one (the record ends before the launch status is
  // read), the destructor on an early `return e`.  Both call end(): it is a no-op on a record that is already closed (open_), and must stay one
  struct Scope {
    Scope(Timing* tm, const char* name, hipStream_t st) : tm_(tm), st_(st) { tm_->begin(name, st_); }
    ~Scope() { tm_->end(st_); }
    Scope(const Scope&) = delete;
    Scope& operator=(const Scope&) = delete;
    hipError_t close() { tm_->end(st_); return hipGetLastError(); }
   private:
    Timing* tm_; hipStream_t st_;
  };
 private:
  bool open_ = false;
};

// Arguments of the per-sequence engine kernels (passed by value).
struct SeqArgs {
  // parameters (device)
  float *lt, *di, *ui, *wh, *bi, *vs, *bs, *wd, *lw;
  int n_item, n_dist, dim;
  // CSR index tables (device)
  const int *off, *p, *q, *dp, *dq;
  int len_max;       // padded row length of the reference tables (analytic padding-row decay)
  int cap;           // capacity in steps of the per-workgroup scratch (>= longest sequence)
  // launch
  const int* uidx;
  int n_seq;
  float* out;        // spatial: 5 per sequence; plain: 1 per sequence
  // scratch (owned by poi_ctx)
  float* ws; size_t ws_stride;      // per-workgroup activations
  float* slab;                      // per-workgroup dense-gradient slabs
  float *g_lt, *g_di;               // zero-initialised gradient tables
  int *mult_lt, *nseq_lt, *mult_di, *nseq_di;
  // predict outputs (row k of the launch goes to output row out_row[k], or k when out_row is null)
  float *hts, *sts; const int* out_row;
  const int* kc_dev; // tile launches: {slabs of the other regions, slabs of the d ui region}, written by te_wgrad (null: n_slab)
  float bcap;        // batch rule: at most `bcap` of the touching sequences' updates count (1 = mean rule), include/poi_hip.h
};

// te_wgrad's (job, K-chunk) grid: `slots` workgroups, nui d ui jobs contracting over P rows and (jobs - nui) jobs over T rows.  Every
// workgroup should get the same number of rows: n_o chunks for the T-row jobs, n_u ~ n_o * P / T for the ui jobs, filling `slots`.
__host__ __device__ inline void te_wgrad_split(int slots, int nui, int jobs, int P, int T, int* n_o, int* n_u, bool xcd = true) {
  float rho = (T > 0 && P > 0) ? (float)P / (float)T : 1.f;
  rho = rho < 0.02f ? 0.02f : rho > 1.f ? 1.f : rho;
  int o = (int)((float)slots / ((float)nui * rho + (float)(jobs - nui)));
  if (o < 1) o = 1;
  int u = (int)((float)o * rho + 0.5f);
  if (u < 1) u = 1;
  while (o > 1 && nui * u + (jobs - nui) * o > slots) --o;
  // A chunk count that is a multiple of 8 puts the T-row jobs of one K-chunk on ONE XCD (workgroup ids go round the 8 XCDs and the
  // jobs of chunk kc sit n_o ids apart): they stream the same h / r*h rows at the same time, so four of the five reads of every H row hit
  // that XCD's L2 instead of HBM.  The slots this frees go to the d ui jobs.
  // (Only where it costs little: at >= 64 chunks the rounding lengthens a chunk by < 11 %; the d ui jobs never get more chunks than
  // the T-row jobs, which is what the slabs are sized for.)
  if (xcd && o >= 64) {
    o &= ~7;
    const int uu = (slots - (jobs - nui) * o) / (nui > 0 ? nui : 1);
    if (nui > 0 && uu > u) u = uu < 2 * u ? uu : 2 * u;
    if (u > o) u = o;
    if (u >= 16) u &= ~7;          // (the d ui jobs of one chunk gather the same POI rows: same XCD for them too)
  }
  *n_o = o; *n_u = u;
}

// Layout of one dense-gradient slab (offsets in floats).
struct DenseLayout { int ui, wh, bi, vs, bs, wd, sur, upq, total; };
__host__ __device__ inline DenseLayout dense_layout(int D, int XW, int NB) {
  DenseLayout l;
  l.ui = 0;
  l.wh = l.ui + 3 * D * XW;
  l.bi = l.wh + 3 * D * D;
  l.vs = l.bi + 3 * D;
  l.bs = l.vs + NB * D;
  l.wd = l.bs + NB;
  l.sur = l.wd + 1;
  l.upq = l.sur + 1;
  l.total = (l.upq + 1 + 3) & ~3;
  return l;
}

// Arguments of the tile engine (tile_engine.hip).
struct TeArgs {
  float *lt, *di, *ui, *wh, *bi, *vs, *bs, *wd, *lw;
  int n_item, n_dist, dim;
  const int *off, *p, *q, *dp, *dq;
  int len_max;
  const int* uidx;
  int n_seq;
  float* out;
  int predict;                        // 1: forward over all L positions, no bookkeeping
  int spatial, xw;                    // 1 / 2D: Distance2Pre (POI + distance-bin input); 0 / D: plain GRU + BPR (n_dist == -1)
  int lt_f16;                         // the POI table `lt` is stored as IEEE half (float32 arithmetic): config X
  int rec32;                          // streaming recurrent kernels on 32-sequence tiles (D = 256; D = 128 on request)
  int bintab;                         // spatial && D >= 128: distance-bin half through per-bin tables (te_ztab / te_dsum)
  float *ztab, *dpart, *dsum, *dgd;   // (n_dist+1) x 3D table; per-chunk partial sums of DA; per-bin sums; per-bin d di sums
  int *dch0, *dch1;                   // first 64-entry chunk / first super-chunk of each bin (+ total)
  // hot bins (round 5): on check-in data a few distance bins hold most steps (short hops) - te_psum, which streams every DA row once for the per-POI
  // sums anyway, also adds the rows of the (<= TE_HB) most frequent bins into per-workgroup partials that take the place of those bins' 64-entry chunk
  // partials (dpart); te_dsum then reads only the rows of the remaining bins.  dhot[0] = number of hot bins, dhot[1 .. TE_HB] = their ids,
  // dhot[8 + b] = hot index of bin b or -1 (te_dprep); npw = workgroups of te_psum (= chunk partials of a hot bin); dhot_on: host switch
  int* dhot; int npw, dhot_on;
  int* dcc0;                          // exclusive scan of the COLD bins' chunk counts (+ total): te_dsum's work list
  float* dpart2; int *dnf, *dnf2, *dbn;   // super-chunk partial sums; distinct-sequence counts per chunk / super-chunk / bin
  int dbg;                            // tuning switch (POI_TE_DBG), 0 in production
  int stream_hints;                   // 1: the tile kernels of the exact forward recurrence (dims 64 / 128) store G, H and RH non-temporally (te_rec_fwdx(i)_kernel_nt); option "stream_hints" / POI_TE_DBG bit 16384 (A/B)
  int early_bins; float bin_alpha, bin_lambda;      // the distance-bin chain of the write-back starts on the side stream behind te_wgrad (launch_te_train)
  // packed-row workspace
  int *soff, *row_src, *row_t, *row_p, *row_dp, *row_ab;   // packed row -> CSR position, step index, input table rows (lt, di)
  float *X, *E, *G, *H, *RH, *DH, *DL, *rowloss;   // DL: d logits (T x padded bins)
  float4 *pVsT, *pVs;
  // forward table (te_rec_fwd16<FT>): ptab = lt . ui[:, :D]^T over all n_item + 1 table rows; iota = 0..n_item, then n_item + 1
  float* ptab; const int* iota; int fwd_tab; float* uiP;       // uiP: ui's POI half with gate-interleaved rows
  float4* pUiP3;                      // uiP as bf16 x 3 fragments (te_pack n16 == 4): B operand of te_ptab_s3 (the forward table on split products)
  float* uiT;                         // ui transposed (2D x 3D), K-contiguous B operand of te_gemm_dx
  float4 *pWhT16, *pWhc16, *pWhzr16;  // 16-column fragments (16x16x4 MFMA) for the recurrent kernels
  int rec_split;                      // recurrent kernels on bf16 x 3 split operands (te_rec_fwd16 / bwd16 <SP>)
  int head_split;                     // chunked head (more than 256 bins) on split products: pVsT / pVs hold bf16 x 3 fragments
  int rec1;                           // per-sequence recurrent kernels on the vector ALUs (te_rec_fwd1 / bwd1): small launches
  float* slab;
  int n_slab, n_head, n_kc;
  // the slot sort only feeds te_scatter (the last kernel): it runs on a side stream next to the GEMMs
  hipStream_t side; hipEvent_t ev_slots, ev_sorted;       // side == nullptr: inline on the main stream
  hipEvent_t ev_start, ev_pack;                           // the weight packs of a launch run on the side stream next to its index preparation
  hipEvent_t ev_bwd, ev_fin;                              // te_finalize / te_parts run on the side stream next to te_wgrad / te_gemm_dx
  // (round 6) hot_early: the hot rows' g*h chunk sums (te_hot_reduce: needs the sorted entries, gcoef and H - nothing later) run on the side stream right behind te_head,
  // beside te_rec_bwd, instead of in the tail; the hot-row list is built behind te_segment (te_hotlist) instead of by te_reduce.  Per-POI regrouping only (no per-entry dx rows)
  int hot_early; hipEvent_t ev_hr0, ev_hr1;
  // (round 6) HYBRID recurrences of mid-size launches (hyb != 0; poi_ctx option "hybrid"): a 1563-sequence launch is 98 tiles of 16 - its two recurrences
  // are the 49-step chains of the longest tile on 98 CUs while 158 CUs idle.  The leading hyb_dev[0] (forward) / hyb_dev[2] (backward) sequences of the
  // launch - the longest ones of a length-sorted launch - run on the per-sequence kernels (te_rec_fwd1x / te_rec_bwd1: 2.0 / 1.0 us per step, persistent
  // grids of hyb_dev[1] / hyb_dev[3] workgroups on stream side2) WHILE the shorter rest runs in 16-sequence tiles (4.5 / 2.9 us per step) on the other CUs;
  // the split is chosen per launch ON THE DEVICE from the launch's own lengths (te_hybrid_kernel: min over the tile boundaries of max(chain of the
  // tiles' longest sequence, steps of the leading sequences / free CUs)).  pWhc1 / pWhzr1: the plain transposes te_rec_bwd1 reads (its own buffers: the
  // tile kernel's bf16 x 3 fragments live in pWhc16 / pWhzr16 at the same time)
  int hyb, hyb_force; int* hyb_dev; float4 *pWhc1, *pWhzr1;      // hyb_force > 0 (option "hybrid_force", tests): that many leading sequences, whatever the cost model says
  hipStream_t side2; hipEvent_t ev_h0, ev_h1, ev_h2, ev_h3;      // (forward fork / join, backward fork / join: an event is never re-recorded inside a launch)
  float *bi_part, *fin_part;           // per recurrent tile d bi partials (n_tile x 3D); per te_finalize block loss sums
  float* hslab; int hstride;          // te_head's per-workgroup d bs | d wd partials (n_head x hstride)
  DenseLayout dl;
  int *mult_lt, *nseq_lt, *mult_di, *nseq_di;    // only the padding rows' entries are used (analytic touches)
  float *hts, *sts; const int* out_row;     // predict: row k of the launch -> output row out_row[k] (null: k)
  // sorted segmented scatter (te_scatter.hip): every table touch of the launch becomes one (row key,
  // entry) pair; a stable radix sort groups them by row, and each row's update is a plain ordered sum
  int key_bits;                       // bits of the largest key (= sentinel = number of table rows)
  int *keys0, *keys1, *vals0, *vals1; // sort ping-pong (key = unified row id, value = slot)
  int *code, *slot_seq;               // per slot: entry code, sequence index in the launch
  int *ent;                           // sorted entry codes (bit 31: first entry of its sequence in the row)
  int *seg_start, *seg_end;           // per unified row: [start, end) in `ent`; end == 0 <=> untouched (persistent, re-zeroed)
  int *hist;                          // radix histogram (bins x blocks)
  int *cnt;                           // [0] number of slots, [1] hot rows, [2] hot chunks, [3] touched rows (urow), [4] S rows, [5] dx entries of the POI rows
  int *urow;                          // list of touched table rows (null: te_reduce scans the tables), see te_segment
  int4* hot_rows;                     // {row, start, count, first chunk}
  int2* hot_chunks;                   // {hot row index, chunk index}
  float* hot_part;                    // (hot chunks, D) partial sums
  int* hot_nf;                        // per hot chunk: distinct-sequence count
  float* gcoef;                       // per packed row: d loss / d (h . e) (te_head)
  float bcap;                         // batch rule cap (see SeqArgs)
  // per-POI regrouping (ppoi; bintab only): the step input lt[p_t] takes far fewer distinct values than there are steps (231 k steps hit
  // ~45 k POIs per launch), and everything the backward pass needs from it is linear in S[p] = sum over the steps with p_t = p of DA_t:
  //   d lt[p] (dx part) = S[p] . ui[:, :D]   (te_gemm_dx over S rows)      d ui[:, :D] = S^T . lt[rows of S]   (te_wgrad, K = S rows)
  int ppoi;
  int *pmark;                         // per lt row: has a dx entry in this launch (zero between launches; te_slots sets, the write-back clears)
  int *urow_p;                        // S row -> lt row (lt row -> S row + 1 is pmark itself after te_passign)
  int *pblk;                          // per-block counts of the scan (S rows | dx entries)
  const int *ks;                      // sorted keys (set by launch_te_sort)
  int *dxe, *dxs, *dstart;            // compacted dx entries of the POI rows: packed step row, S row; first list position of every S row (+ end)
  float *S, *pfirst, *plast;          // S (rows x 3D); per 64-entry range: sum of its opening / closing run
  int wg_slots;                       // te_wgrad: workgroups of the (job, K-chunk) grid (2 per CU)
  int* kc_dev;                        // {K-chunks of the non-ui jobs, of the d ui jobs}: chosen ON THE DEVICE from the launch's own S-row / step counts
                                      // (te_wgrad_split) - the split-K order is a function of the launch alone, not of its history
  unsigned sr_salt;                   // != 0: a half POI table is written back with stochastic rounding (poi_ctx_set_f16_rounding), salt of this launch
  const float* zrow;                  // resident all-zero row (>= 2 * dim floats), never written: target of branch-free "no contribution" loads
  // exact forward (te_xfwd.hip): input product + forward recurrence in ~40-bit fixed point on the int8 matrix cores, float64 gate math
  int xcomp; int *xidx, *xlist, *xblk, *xcnt, *row_pc;      // exact forward table over the launch's step-input POIs only (te_xcount / te_xassign): lt row -> table row, table row -> lt row, per-block counts, row count, per-step table row
  int efuse;                          // (round 6) te_head3 gathers E = lt[p'] - lt[q'] itself (row_pq: the step's positive / negative POI): no E rows in HBM, te_gather only translates ids; dim 128, training, <= 256 bins; POI_TE_EFUSE
  int2* row_pq;
  int xrec1;                          // the recurrence of every sequence in its own workgroup on the float64 vector ALUs (te_rec_fwd1x): small launches
  int xfwd, xft;                      // on; pre-activations from the forward table ptabx[p_t] + ztabx[dp_t] (else gx[row])
  int xid_cap;                        // xft: the recurrence stages the table-row ids of its sequences' steps in LDS, xid_cap steps per sequence (0: it loads them inside the step loop); te_xfwd_ids_cap
  double *gx, *ptabx, *ztabx;         // (T + spare) x 3D per step | (n_item + 1 + spare) x 3D | (n_dist + 1) x 3D, gate-major columns (g D + unit)
  uint4 *xWh8, *xUi8; double *xWhS, *xUiS;      // digit fragments + row scales of wh (16x16x64 order) and of ui's POI half (32x32x32 order)
  int x_rows_est;                     // host-side bound of the packed row count (grid sizing of te_gemmx)
  int* xflag; int xlaunch;            // != launch id: no non-finite weight / input row seen while this launch's operands were prepared (te_xfwd.hip x_flag_bad)
};
// entry code: packed-row index of the position (28 bits) + what the position contributes
#define TE_ENT_ROW 0x0FFFFFFF
#define TE_ENT_DX 0x10000000      // + dx[row] (lt half for POI rows, di half for distance-bin rows)
#define TE_ENT_GH 0x20000000      // + g[row-1] * h[row-1]
#define TE_ENT_NEG 0x40000000     // the g*h term enters with a minus sign (negative sample)
#define TE_ENT_FIRST 0x80000000u  // first entry of its sequence within the row segment
#define TE_HYB_NMAX 4096         // hybrid recurrences: te_scan keeps the launch's step counts in LDS for the split
#define TE_PSUM_WG 1024          // workgroups of te_psum = chunk partials of a hot bin: device-independent (was num_cu * 4)
#define TE_HB 4                   // hot distance bins summed by te_psum (TeArgs.dhot)
#define TE_HOT_BIN_MIN 4096       // ... when they hold at least this many steps of the launch
#define TE_COLD_MAX 64            // rows with more entries are reduced in 256-entry chunks by whole workgroups
#define TE_HOT_CHUNK 64
#define RS_MAXBIN 512
#define RS_GRID 256
#define RS_HIST_INTS (RS_MAXBIN * RS_GRID)   // radix histogram: bins x blocks
bool te_supported(int D, int n_dist);
bool te_bintab(int D, bool spatial, int n_dist);
// distance bins padded for the head / d vs tiles: 32 x {1, 2, 4, 7, 8} up to 256 bins, a multiple of 256 beyond (te_head_big's chunks)
__host__ __device__ inline int te_nbp_dev(int n_dist) {
  const int t = (n_dist + 1 + 31) / 32;
  return t <= 8 ? 32 * (t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 7 ? 7 : 8) : 256 * ((n_dist + 1 + 255) / 256);
}
int te_wgrad_jobs(int D, int n_dist, bool spatial, bool bintab);
hipError_t launch_te_sort(TeArgs& A, hipStream_t st);
hipError_t launch_te_psum(TeArgs& A, int num_cu, hipStream_t st);
hipError_t launch_te_passign(TeArgs& A, hipStream_t st);
hipError_t launch_te_hot_reduce(TeArgs& A, int num_cu, hipStream_t st);      // chunk sums of the hot rows (te_scatter.hip); early on the side stream when TeArgs.hot_early
hipError_t launch_te_dprep(TeArgs& A, hipStream_t st);        // chunk offsets of the distance-bin chain (behind the slot sort; launch_te_bins expects them)      // S rows of the per-POI regrouping (behind the slot sort)
int te_wgrad_ui_jobs(int D, int n_dist, bool spatial, bool bintab);
hipError_t launch_te_scatter(TeArgs& A, float alpha, float lambda, int num_cu, hipStream_t st, Timing* tm, int* forked = nullptr);      // forked: the plan record (poi_ctx_last_plan "fork")
hipError_t launch_te_bins(TeArgs& A, float alpha, float lambda, int num_cu, hipStream_t sb, Timing* tm);      // te_scatter.hip: per-bin sums of DA -> d di, d ui[:, D:]
int te_nbp(int n_dist);
void launch_te_iota(int* buf, int n, hipStream_t st);
hipError_t launch_te_one(TeArgs& A, float alpha, float lambda, int l_cap, hipStream_t st, Timing* tm);      // n_seq == 1, whole step
bool te_one_supported(int D, bool spatial, int max_len);
hipError_t launch_te_train(TeArgs& A, int num_cu, hipStream_t st, Timing* tm);
hipError_t launch_te_predict(TeArgs& A, int num_cu, hipStream_t st, Timing* tm);
bool te_xfwd_supported(int D);
int te_xfwd_ids_cap(int D, int steps, bool per_sequence);      // TeArgs.xid_cap for sequences of at most `steps` steps: steps + 1, or 0 when the id table does not fit the kernel's LDS
hipError_t launch_te_xfwd(const TeArgs& A, int num_cu, hipStream_t st, Timing* tm, int phase);      // te_xfwd.hip: phase 0 = input product, 1 = recurrence
hipError_t launch_te_xsts(const TeArgs& A, int num_cu, hipStream_t st);      // te_xfwd.hip: predict's sts = softmax(vs . hts + bs) in float64 (exact forward)
hipError_t launch_rows_apply(const SeqArgs& A, bool spatial, int grid, float alpha, float lambda, hipStream_t st, Timing* tm);
hipError_t launch_dense_apply(const SeqArgs& A, bool spatial, int n_slab, int n_slab_head, float alpha, float lambda, hipStream_t st, Timing* tm);

size_t seq_ws_floats(int D, int NB, int cap);

// Arguments of the exact (float64) engine, exact_engine.hip: SeqArgs with float64 scratch.  Tables stay float32.
struct ExArgs {
  float *lt, *di, *ui, *wh, *bi, *vs, *bs, *wd, *lw;
  int n_item, n_dist, dim;
  const int *off, *p, *q, *dp, *dq;
  int len_max, cap;
  const int* uidx;
  int n_seq;
  float* out;
  double* ws; size_t ws_stride;     // per-workgroup activations (float64)
  double* slab;                     // per-workgroup dense-gradient slabs (float64)
  double *g_lt, *g_di;              // zero-initialised float64 gradient tables
  int *mult_lt, *nseq_lt, *mult_di, *nseq_di;
  float *hts, *sts; const int* out_row;
  float bcap;
};
size_t ex_ws_doubles(int D, int NB, int cap);
hipError_t launch_ex_train(const ExArgs& A, bool spatial, int grid, double alpha, double lambda, hipStream_t st, Timing* tm);
hipError_t launch_ex_predict(const ExArgs& A, bool spatial, int grid, hipStream_t st, Timing* tm);
hipError_t launch_seq_train(const SeqArgs& A, bool spatial, int grid, float alpha, float lambda, hipStream_t st, Timing* tm);
hipError_t launch_seq_predict(const SeqArgs& A, bool spatial, int grid, hipStream_t st, Timing* tm);

// CA-RNN (carnn.hip)
struct CaArgs {
  float *lt, *wd, *M;                 // POI table (n_item+1, D), interval matrices (n_dist+1, H, D), input matrix (H, D); H == D
  int n_item, n_dist, dim;
  const int *off, *p, *q, *dp, *dq;
  int len_max, cap;
  const int* uidx;
  int n_seq;
  float* out;                         // train: loss per sequence
  float* ws; size_t ws_stride;        // per-workgroup activations
  float* slab;                        // per-workgroup d M
  float *g_lt, *g_wd;                 // zero-initialised gradient tables
  int *mult_lt, *nseq_lt, *mult_wd, *nseq_wd;
  float* hts;                         // predict output
  float bcap;
  // ---- outer-product path (carnn_train2: dims 64 / 128): packed per-step state and the (matrix id, a, b) entries whose sorted,
  // segmented products a (x) b are the gradients of the interval matrices and of M (no float atomics on matrices)
  int* soff;                          // n + 1: packed step offsets (step t of sequence k = row soff[k] + t)
  float* Hpk;                         // (T + n) x D: h_0 .. h_ns of sequence k at rows soff[k] + k + t
  float* EA;                          // T x 5 x D: g mp | -g mq | da | g vp | -g vq of every step
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;      // radix sort of the 6 T entries by matrix id; cnt[0] = 6 T
  int *ent_a, *ent_b;                 // per entry: EA vector (row of D floats), b source (>= 0: Hpk row, < 0: ~row of lt)
  int *seg_start, *seg_end, *chunk_first;               // per matrix id (n_dist + 2 ids: the interval matrices, then M)
  float* partial;                     // per 512-entry chunk: D x D partial product
  int n_chunk_cap;
  float* PM;                          // (n_item + 1) x D: lt . M^T, the input product of every POI (computed once per launch)
  // gradient of the POI rows: d lt[row] = M^T (sum of the step vectors that name the row) - three entries (row, EA vector) per step,
  // sorted by row; 64-entry windows of the sorted list are summed per run (vpart), a wave per row adds its runs in order
  int *k2a, *k2b, *v2a, *v2b;         // radix sort of the 3 T row entries (cnt[1] = 3 T)
  int *seg2_start, *seg2_end;         // per POI row (n_item + 2)
  float* vpart;                       // 3 T x D: partial sums, stored at the sorted position of a run's first entry inside its window
};
size_t carnn_ws_floats(int D, int cap);
hipError_t launch_carnn_train2(const CaArgs& A, int grid, float alpha, float lambda, hipStream_t st, Timing* tm);
// stable LSD radix sort of (keys, element index) pairs on `bits` key bits; n_ptr[0] = element count (device).  *ks / *vs: the buffers
// that hold the sorted keys / the original indices in sorted order.  hist: RS_HIST_INTS + RS_MAXBIN ints.
hipError_t launch_radix_sort(int* keys0, int* keys1, int* vals0, int* vals1, const int* n_ptr, int bits, int* hist, hipStream_t st,
                             const int** ks, const int** vs);
hipError_t launch_carnn_train(const CaArgs& A, int grid, float alpha, float lambda, hipStream_t st, Timing* tm);
hipError_t launch_carnn_predict(const CaArgs& A, int grid, float* wrs, hipStream_t st, Timing* tm);
hipError_t launch_carnn_score(const float* users, const float* items, const float* M, const float* dists, const double* coords, const double* cphi,
                              const double* thr, const int* last_poi, int n, int N, int n_dist, int D, double dd, float* scratch, float* out,
                              hipStream_t st, Timing* tm);

// BPR-MF
struct BprArgs {
  float* ux; void* lt;    // lt: float32, or IEEE half when lt_f16 (float32 arithmetic; config X's table storage)
  int lt_f16; unsigned sr_salt;      // != 0: stochastic rounding of the half write-back (poi_ctx_set_f16_rounding)
  int n_user, n_item, dim;
  const int *uidx, *p, *q;
  int n;
  float alpha, lambda;
  float* loss;
  int* bad;               // device counter of out-of-range ids (poi_ctx_take_bad_ids)
  float bcap;             // batch rule cap (see SeqArgs)
  // snapshot mode (bpr.hip): 3 n table touches sorted by row
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;
  const int *ks, *vs;     // sorted keys / touch ids (set by launch_bpr)
  int4* meta;             // per 64-touch window: {touches of its opening run, that run goes on, touches of its closing run, its row}
  float *g;               // per triple: d loss / d u
  float *shadow;          // (n_user, D): new user rows until the POI pass has read the entry values
  float *lead, *trail;    // per window: partial sum of its opening / closing run
};
hipError_t launch_bpr(BprArgs& A, int mode, int num_cu, hipStream_t st, Timing* tm);

// FPMC-LR (fpmc.hip)
struct FpmcNbrArgs {
  const double *coords, *cphi;      // (n, 2) lat, lon; cos(lat * pi / 180) per POI (data.cos_lat)
  const int* order;                 // POI ids in ascending latitude
  int n;
  double c_ud, band_deg;            // neighbour <=> c < c_ud; latitude half-width of the scanned band (degrees)
  long long* off;                   // (n + 1): counts pass writes the offsets; fill pass reads them
  int* nbr;                         // fill pass output
};
hipError_t launch_fpmc_neighbors(FpmcNbrArgs& A, int fill, hipStream_t st);
hipError_t launch_fpmc_sample(const long long* off, const int* nbr, const int* pos, long long n, int n_item, unsigned long long seed, int* out,
                              hipStream_t st);
struct FpmcArgs {
  float *ui, *iu, *ia, *ai;         // (n_user, D), 3 x (n_item + 1, D)
  int n_user, n_item, dim;
  const int *u, *a, *i, *j;
  int n;
  float alpha, lambda, bcap;
  float* loss;
  int* bad;                         // device counter of rejected transitions (poi_ctx_take_bad_ids)
  int sentinel;                     // key of a rejected transition's touches: n_user + 3 (n_item + 1), sorts last
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;      // radix sort of the 6 n touches
  const int *ks, *vs;
  int4* meta;                       // per 64-touch window: {opening run's touches, it goes on, closing run's touches, its key}
  float *s, *lead, *trail, *slot;   // per transition sigmoid(-x); per-window partial sums; (6 n, D) new rows at a run's first position
};
hipError_t launch_fpmc_step(FpmcArgs& A, int num_cu, hipStream_t st, Timing* tm);

// PRME (prme.hip)
struct PrmeArgs {
  float *du, *dp, *ds;              // (n_user, D), 2 x (n_item + 1, D)
  int n_user, n_item, dim;
  const int *u, *p, *q, *prev, *gap;
  const double* d;
  int n, thd;
  float alpha, lambda, bcap, cw;
  float* loss;
  int* bad;                         // device counter of rejected transitions (poi_ctx_take_bad_ids)
  int sentinel;                     // key of a lost occurrence / a rejected transition's touches: n_user + 2 (n_item + 1), sorts last
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;      // radix sort of the 7 n touches
  const int *ks, *vs;
  int4* meta;                       // per 64-touch window: {opening run's touches, it goes on, closing run's touches, its key}
  float *ga, *gb, *lead, *trail, *slot;   // per transition 2 a g, 2 b g; per-window partial sums; (7 n, D) new rows at a run's first position
};
hipError_t launch_prme_step(PrmeArgs& A, int num_cu, hipStream_t st, Timing* tm);
struct PrmeScoreArgs {
  const float *du, *dp, *ds;        // (n_user, D), (>= n_item, D), (n_item + 1, D)
  const double* coords;             // (n_item + 1, 2) lat, lon (row n_item: the pad POI)
  const int *users, *qpoi;          // per output row: user, query POI in [0, n_item]
  int n_rows, n_user, n_item, dim, k;      // k > 0: fused top-K
  float cw;
  float* out;                       // (n_rows, n_item) when k == 0
  int* idx_out; float* sc_out;      // (n_rows, k) when k > 0 (sc_out may be NULL)
};
hipError_t launch_prme_score(PrmeScoreArgs& A, hipStream_t st);

// GeoIE (geoie.hip)
struct GeoieArgs {
  float *g, *h, *t, *z;             // (n_item + 1, D) x 3, t (n_user, D)
  double* ab;                       // a, b on the device
  int n_user, n_item, dim;
  const int *off, *p, *q, *users;   // training CSR (n_user + 1 offsets), launch users (n)
  const double *coords, *cphi;      // (n_item, 2) lat, lon; cos(lat * pi / 180) per POI
  int n, P;                         // launch users, host total of rows sum max(L - 1, 0)
  long long n_pairs;                // host total of pairs (poi_geoie_pair_distances), -1 in the step
  double d_min;
  float alpha, lambda, bcap;
  float* loss;                      // (n) per user
  int* bad;                         // device counter of rejected users (poi_ctx_take_bad_ids)
  int sentinel;                     // key of a rejected user's touches: 3 (n_item + 1), sorts last
  int *rowoff, *troff, *tcoff;      // (n + 1) exclusive scans of rows, row-pass tiles, column-pass tiles
  long long* pairoff;               // (n + 1) pairs (pair distances only)
  int *ubad, *tot;                  // per-user rejection flag; {rows, row tiles, column tiles, -, totals mismatch}
  int* tuser;                       // (P) launch user of a row
  float* coef;                      // (P) sigmoid(-diff_i) / (i + 1)
  double *rloss, *rda, *rdb, *uda, *udb;      // per row / per user: loss, d cost / d a, d cost / d b
  float* G;                         // (3 P, D) loss gradients of the g touches [0, P) and the h touches [P, 3 P)
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;      // radix sort of the 5 P touches
  const int *ks, *vs;
  int4 *meta, *meta2;               // per 64-touch window: {opening run's touches, it goes on, closing run's touches, its key}; {users of both}
  float *lead, *trail, *slot;       // per-window partial sums; (5 P, D) new rows at a run's first position
  float *dp_out, *dq_out;           // packed pair distances
};
hipError_t launch_geoie_step(GeoieArgs& A, int num_cu, hipStream_t st, Timing* tm);
hipError_t launch_geoie_pairs(GeoieArgs& A, int num_cu, hipStream_t st);
hipError_t launch_geoie_uvec(const float* g, const float* t, const int* off, const int* p, int n_user, int n_item, int dim, int len_max,
                             int norm, float* out, int num_cu, hipStream_t st);

// GeoIE scoring under the trained rule (geoie_score.hip)
#define GEO_K_MAX 32                        // list length (one half wave)
struct GeoScoreArgs {
  const float *g, *h, *z; const double* ab; // (n_item + 1, D) x 3; a, b on the device
  int n_item, dim;
  const int *off, *p, *mult;                // compacted histories: CSR of distinct ascending ids, their multiplicities (null = 1 each)
  const int* rows; const float* tu;         // (n_rows) histories of the CSR (null = identity); (n_rows, D) user rows (null = zero)
  int n_rows;
  const double *coords, *cphi; double d_min;
  int span, n_split;                        // candidates per workgroup; workgroups per row = ceil(n_item / span)
  float* out;                               // matrix mode (k == 0): (n_rows, n_item)
  int k; const int *ex_off, *ex;            // top-K mode: per-row exclusion lists (null = none)
  int* idx_out; float* score_out; int* count_out;             // score_out / count_out may be null
  float* part_s; int *part_i, *part_cnt;    // n_split > 1: (n_rows, n_split, GEO_K_MAX) partial lists, (n_rows, n_split) counts
  int* bad;                                 // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_geoie_score(GeoScoreArgs& A, hipStream_t st, Timing* tm);

// POI2Vec (poi2vec.hip)
struct P2vArgs {
  float *xu, *wl, *pb;              // (n_user, D), (n_item [+ pad], D), (n_node, D)
  const int* routes; const signed char* lrs; const float* probs; const int* rid;      // (n_item + 1, 4, depth) x 2, (n_item + 1, 4) x 2
  int n_user, n_item, n_node, depth, dim;
  const int *off, *tgt, *coff, *cidx, *users;      // CSR of CSR: user -> positions -> context POIs; launch users (n)
  int n, n_pos, n_ctx, len_max, n_tile;            // host totals of the launch's positions and context entries; 64-item tiles
  float alpha, lambda, bcap;
  float* loss;                      // (n) upq per user
  int* bad;                         // device counter of rejected users (poi_ctx_take_bad_ids)
  int *ubad, *acc, *lpos, *lctx, *tot, *cnt;       // per user: bad flag, accepted, position / context offsets; {mismatch, k}; sort counts
  float* pmax; double* psum;        // (n, n_tile) per-tile max / sum of exp of the logits
  double *posval, *gz, *cbuf, *gcbuf, *lse, *tsum; // per position: s_t + log paths, (4 depth) d / d z, c_i, d / d c_i; per user: lse, sum of target rows
  float *scale, *dxu;               // alpha min(k, cap) / k; (slots, n, D) partial sums of dXU
  int *keys0, *keys1, *vals0, *vals1, *k2a, *k2b, *v2a, *v2b, *epos, *hist;
  const int *ks, *vs, *k2s, *v2s;
};
struct P2vScoreArgs {
  const float *xu, *wl, *pb, *probs; const int *rid, *leaf_nodes, *users, *coff, *cidx;
  int n_user, n_item, n_node, depth, dim, n_batch, length, n_rows, axis, k;
  double *cl, *zf, *rp, *ssum; float *logit, *smax, *out, *score_out; int* idx_out;
  const int *ex_off, *ex; int* count_out;      // top-K only (poi_poi2vec_topk_ex): per-row exclusion lists, ascending unique ids; candidates ranked.  NULL otherwise
};
hipError_t launch_poi2vec_step(P2vArgs& A, int num_cu, hipStream_t st, Timing* tm);
hipError_t launch_poi2vec_scores(P2vScoreArgs& A, int num_cu, hipStream_t st, Timing* tm);

// Mini-batch Lstm / Rnn cells (cells.hip)
#define CELL_NT 256               // threads of the recurrent workgroup (one sequence per workgroup)
#define CELL_GRID_MAX 512         // bound of the persistent recurrent grid: device-independent (two workgroups per CU on 256 CUs)
#define CELL_DENSE_CHUNKS 64      // row chunks of the dense-gradient contraction (partials added in chunk order)
#define CELL_PART 1024            // LDS doubles for the split contractions' partial sums
struct CellArgs {
  float *lt, *ui, *wh, *bi;         // (n_item + 1, D); (G, D, D) x 2; (G, D)
  int n_item, dim, G;               // G = gate blocks: 1 Rnn, 4 Lstm (POI_CELL_*)
  const int *off, *p, *q;
  int n_user, len_max, max_len;
  const int *uidx, *out_row;
  int n_seq;
  float *out, *hts;                 // train: loss per sequence; predict: (n, D)
  double alpha, lambda;
  int grid, ch_rows;                // workgroups of the recurrent kernel; position rows per dense-gradient chunk
  int* bad;                         // device counter of rejected sequences (poi_ctx_take_bad_ids)
  int *slen, *poff, *cnt, *rowp;    // per sequence: L (0: rejected), first position row; cnt = {entries, rows, pad multiplicity, rejected}; per row: p_t
  int *keys0, *keys1, *vals0, *vals1, *hist;      // radix sort of the 2 P + 1 row entries
  const int *ks, *vs;
  float4 *uiP, *whP, *uiT, *whT;    // weights packed for the forward / backward contractions (cell_pack_kernel)
  double *H, *ACT, *CS, *DX, *gam;  // per position row (see cells.hip)
  double *dpart, *lead, *trail;     // dense-gradient chunk partials; per 64-entry window: partial sum of its opening / closing run
  int4* meta; int* mm;              // per window: {opening run's multiplicity, it goes on, closing run's entries, its row}; closing run's multiplicity
  float* slot;                      // (2 P + 1, D) new rows at a run's first sorted position
};
size_t cell_lds_bytes(int D, int G);
int cell_grid(int n_seq, int cap);
int cell_chunk_rows(int n_seq, int max_len);
hipError_t launch_cell_step(CellArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_cell_predict(CellArgs& A, hipStream_t st, Timing* tm);

// VBPR (vbpr.hip)
#define VBPR_DENSE_CHUNKS 64      // at most this many row chunks of the dense-gradient contraction (partials added in chunk order)
struct VbprArgs {
  float *ux, *lt, *ue, *ei;         // (n_user, D), (n_item + 1, D), (n_user, D), (D, F)
  const float* fi;                  // (n_item + 1, F), never written
  int n_user, n_item, dim, n_img;
  const int *uidx, *p, *q;
  int n;
  float alpha, lambda, lambda_ev, bcap;
  float* loss;
  int* bad;                         // device counter of rejected triples (poi_ctx_take_bad_ids)
  int sentinel;                     // key of a rejected triple's touches: 2 n_user + n_item + 1, sorts last
  int *keys0, *keys1, *vals0, *vals1, *hist, *cnt;      // radix sort of the 4 n touches; cnt = {4 n, accepted triples}
  const int *ks, *vs;
  int4* meta;                       // per 64-touch window: {opening run's touches, it goes on, closing run's touches, its key}
  int *okf, *ord;                   // per triple: accepted; accepted triples in launch order
  float *g, *V;                     // per triple: d loss / d x; ei (fi[p] - fi[q])
  float *lead, *trail, *slot;       // per-window partial sums; (4 n, D) new rows at a run's first sorted position
  double* dpart;                    // (n_chunk, D, F) partial sums of d ei
  int ch_rows, n_chunk;             // accepted triples per chunk, chunks: vbpr_chunking(n)
  int grid_cap;                     // option "vbpr_grid": at most this many workgroups per kernel (0: none)
  float* out; int n_rows;           // items: (n_rows, 2 D) output over the n_rows = n_item + 1 table rows
};
void vbpr_chunking(int n, int* ch_rows, int* n_chunk);
hipError_t launch_vbpr_step(VbprArgs& A, int num_cu, hipStream_t st, Timing* tm);
hipError_t launch_vbpr_items(VbprArgs& A, int num_cu, hipStream_t st, Timing* tm);
hipError_t launch_vbpr_users(const float* ux, const float* ue, int n_user, int dim, float* out, int num_cu, hipStream_t st, Timing* tm);

// Online sessions (session.hip): per-slot recurrent state advanced one check-in at a time
#define SESS_TILE_LDS_MAX (152 * 1024)      // dynamic LDS the tile kernel may ask for (opt-in per device)
#define SESS_EVENT_GRID_MAX 16384           // workgroups of the event kernel (it strides over larger launches)
#define SESS_SCAN_MAX 256                   // event path: up to this many events a workgroup scans the call's slots for repeats itself
struct SessArgs {
  const void* lt; int lt_f16;               // POI snapshot: float32, or IEEE half when lt_f16
  const float *di, *ui, *wh, *bi, *vs, *bs; // di / vs / bs null: the plain cell
  int n_item, n_dist, dim, xw, spatial;     // xw = D or 2 D columns of ui
  const double *coords, *cphi, *thr; double dd;
  double* h; float* sts; int *last_poi, *steps; int n_slot;      // the state, updated in place
  const int *slot, *poi; int n;
  float *hts_out, *sts_out;                 // optional (n, D) / (n, n_dist + 1) copies of the new rows (NaN rows: rejected events)
  int* bad;                                 // device counter of rejected events (poi_ctx_take_bad_ids)
  int* owner;                               // (n_slot) scratch of the repeated-slot check, or null: the event kernel scans the call
  int head_only;                            // poi_session_sts: softmax(vs . h[slot] + bs) to sts_out, nothing else
};
size_t sess_tile_lds(int D, int xw, int NB, int spatial);
size_t sess_event_lds(int D, int xw, int NB, int spatial);
bool sess_tile_supported(int D, int xw, int NB, int spatial);
hipError_t launch_session(SessArgs& A, int tile, hipStream_t st, Timing* tm);
// the repeated-slot claims alone (sess_claim_kernel + sess_mark_kernel): owner[s] = the one event that names slot s, or -1
hipError_t launch_session_claims(const int* slot, int n, int n_slot, int* owner, hipStream_t st);

// Leave-one-out attribution (explain.hip): base and per-variant scores of listed POIs, 16 (row, key) columns per workgroup
#define EXPLAIN_C_MAX 32                    // listed POIs per row
struct ExplainArgs {
  const void* lt; int lt_f16;               // POI snapshot: float32, or IEEE half when lt_f16 (step inputs and the scored rows)
  const float *di, *ui, *wh, *bi, *vs, *bs, *wd;      // di / vs / bs / wd null: the plain cell
  int n_item, n_dist, dim, xw, spatial;
  const double *coords, *cphi, *thr; double dd;
  const int *h_off, *h_ids; long long total;          // histories: row r = h_ids[h_off[r] .. h_off[r + 1]), total ids
  const int *grp, *g_off; int n_group;      // group of every position within its row; rows of delta per row: g_off[r] .. g_off[r + 1]
  int n;
  const int *base_cols, *var_cols; int n_var;         // int4 (row, key, start, 0) per column: n base columns (key -1), n_var variants
  int start_mode;                           // 1: a variant starts at its column's start from the checkpoint; 0: at position 0 from h = 0
  double* ck; int nck;                      // (n, nck, D) base states after positions 16, 32, ..., 16 nck
  int* rowbad;                              // (n) rows with an id out of range
  const int* lists; int C;                  // (n, C), -1: no entry
  double *base, *delta;                     // (n, C), (n_group, C)
  double *h_out, *sts_out; int* last_out;   // optional per variant: (n_group, D), (n_group, n_dist + 1), (n_group)
  int* bad;                                 // device counter of rejected rows (poi_ctx_take_bad_ids)
};
bool explain_supported(int D, int xw, int NB, int spatial);
hipError_t launch_explain(ExplainArgs& A, hipStream_t st, Timing* tm);

// Online sessions of Lstm / Rnn / CA-RNN (session_cells.hip): the same state and launch regimes, templated on the cell
struct SessCellArgs {
  int G;                                    // gate blocks: 1 Rnn, 4 Lstm, 0 CA-RNN
  const float *lt, *ui, *wh, *bi;           // cells: ui / wh (G D, D), bi (G D).  CA-RNN: ui = M (D, D), wh = wd (n_dist + 1, D, D), bi null
  int n_item, n_dist, dim;                  // n_dist: CA-RNN only
  const double *coords, *cphi, *thr; double dd;      // CA-RNN only
  double *h, *c; int *last_poi, *steps; int n_slot;  // the state, updated in place (c: Lstm only)
  const int *slot, *poi; int n;
  float* hts_out;                           // optional (n, D) copy of the new rows (NaN rows: rejected events)
  int* bad;                                 // device counter of rejected events (poi_ctx_take_bad_ids)
  int* owner;                               // (n_slot) scratch of the repeated-slot check, or null: the event kernel scans the call
  const double* wrs;                        // CA-RNN tile path: (n_dist + 1, D) float64 row sums of wd, written by the launch's pre-pass
};
size_t sess_cell_tile_lds(int G, int D);
size_t sess_cell_event_lds(int G, int D);
bool sess_cell_tile_supported(int G, int D);
hipError_t launch_session_cells(SessCellArgs& A, int tile, hipStream_t st, Timing* tm);

// Restricted top-K (near.hip): candidates within a radius of an anchor POI, minus a per-row exclusion list
#define NEAR_K_MAX 32                       // list length (one half wave)
#define NEAR_SPLIT_LIMIT 64                 // workgroups a row's band may be split over
struct NearArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k;
  const double *coords, *cphi; const int* order;             // null when no row has a radius test or a distance term
  const int* anchor; double c_r, band_deg;                    // c_r = +inf: no radius test
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  const float *wd, *sts; const double* thr; int n_dist; float bin_scale;      // distance term, or wd null
  int n_split;                                                // workgroups per row (1 on the row path)
  float* part_s; int *part_i, *part_cnt;                      // split path: (n, n_split, NEAR_K_MAX) partial lists, (n, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // score_out / count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_near(NearArgs& A, hipStream_t st, Timing* tm);

// What every kernel that walks 32-row x 32-item tiles of users . items takes (rank.hip, group.hip, route.hip, diverse.hip).  The host
// checks and fills it in one place (tile_operands, abi_serve.hip) and copies it into the family's argument struct, which holds the same
// members in an order of its own: behind a common base the tile walks compiled to slower code (route's distance-term walk by 3 - 4 %)
struct TileOperands {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *ex_off, *ex;                                     // per-row (group, list) exclusion lists (ascending ids), or both null
  int* bad;                                                   // device counter of rejected rows / groups / targets (poi_ctx_take_bad_ids)
};

// The partial top-K lists of a split path and where their fold goes (topk_merge.hip): row r owns the lists r n_split .. of k_max entries
struct SliceLists {
  const float* part_s; const int *part_i, *part_cnt; int n_split, k;
  int* idx_out; float* score_out; int* count_out;             // (rows, k); score_out / count_out may be null
};
void launch_topk_slices_merge(const SliceLists& L, int k_max, int n_rows, hipStream_t st);      // k_max (the lists' length): 32 or 64
template <class Args>
inline SliceLists slice_lists(const Args& A) { return SliceLists{A.part_s, A.part_i, A.part_cnt, A.n_split, A.k, A.idx_out, A.score_out, A.count_out}; }

// Exact rank of target POIs among all POIs (rank.hip)
#define RANK_LT_MAX 8                       // targets per row
#define RANK_TILES_MAX 65535                // item tiles one wave may walk: its per-lane counters are 16 bits wide
struct RankTgt { float s; int id; };        // a target's score and id; (+inf, -1): not ranked
struct RankArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, len_t;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *tgt, *tmask;                                     // (n, len_t)
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  int n_split;                                                // item ranges (one per wave) of a 32-row tile
  int t_off;                                                  // first target slot of this walk (pass 2 takes up to 4 per launch)
  RankTgt* tl;                                                // workspace (32-row tiles, RANK_LT_MAX): pass 1 -> pass 2
  int* rank_out; float* score_out; int* count_out;            // score_out / count_out may be null
  int* bad;                                                   // device counter of rejected targets / rows (poi_ctx_take_bad_ids)
};
hipError_t launch_rank(const RankArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_rank_scores(const float* scores, int n, int n_item, const int* tgt, const int* tmask, int len_t, const int* ex_off,
                              const int* ex, int* rank_out, int* count_out, int* bad, hipStream_t st);

// Group recommendation (group.hip): top-K of an aggregate (mean / least misery) of the members' scores
#define GROUP_K_MAX 32                      // list length (one half wave)
#define GROUP_GPT 8                         // groups a workgroup owns; it packs them into passes of at most 32 member rows
#define GROUP_SPLIT_LIMIT 64                // workgroups the item range may be split over
struct GroupArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k, n_grp, agg;                          // agg: 0 mean, 1 least misery
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *g_off, *g_mem;                                   // CSR of the groups' member rows
  const int *ex_off, *ex;                                     // per-group exclusion lists (ascending ids), or both null
  int n_split;                                                // item slices, one workgroup each (1 on the tile path)
  float* part_s; int *part_i, *part_cnt;                      // split path: (n_grp, n_split, GROUP_K_MAX) partial lists, (n_grp, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // score_out / count_out may be null
  int* bad;                                                   // device counter of rejected groups (poi_ctx_take_bad_ids)
};
hipError_t launch_group(GroupArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_group_scores(const float* scores, GroupArgs& A, hipStream_t st, Timing* tm);

// Audience recommendation (audience.hip): the top-K candidate rows (users) of each query POI - tile_walk.h's walk with the axes swapped
#define AUDIENCE_K_MAX 32                   // list length (one half wave)
#define AUDIENCE_NDIST_MAX 1024             // distance bins whose thresholds fit the walk kernel's LDS beside its lists
struct AudienceArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int* pois; int n_q;                                   // the query POIs
  const int *ex_off, *ex;                                     // per-query exclusion lists (ascending row indices), or both null
  int n_split;                                                // slices of the user range, one workgroup each per 32-query block
  float* part_s; int *part_i, *part_cnt;                      // split regime: (n_q, n_split, AUDIENCE_K_MAX) partial lists, (n_q, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // (n_q, k); score_out / count_out may be null
  float* rows_out; long long ld;                              // poi_audience_rows: rows_out[q * ld + u], ld >= n
  int* bad;                                                   // device counter of rejected queries (poi_ctx_take_bad_ids)
};
hipError_t launch_audience(const AudienceArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_audience_rows(const AudienceArgs& A, hipStream_t st, Timing* tm);

// Similar rows (similar.hip): the top-K rows of ONE table most similar to each query row - tile_walk.h's walk along the streamed rows, the table on both
// sides and a float64 similarity epilogue; the nearest history POI of every listed POI
#define SIMILAR_K_MAX 32                    // list length (one half wave)
struct SimilarArgs {
  const void* x; int x_f16;                                   // (n, dim) float32 or IEEE half: the table, on both sides
  int n, dim, k;
  const double* inv;                                          // (n) 1 / |x_i|, 0 for a zero row (row_inv_norms_kernel)
  const double *coords, *cphi; double g, omg, scale_km;       // geographic part (coords null: g == 0); omg = 1 - g
  const int* queries; int n_q;                                // the query rows
  const int *ex_off, *ex;                                     // per-query exclusion lists (ascending row indices), or both null
  int n_split;                                                // slices of the row range, one workgroup each per 32-query block
  float* part_s; int *part_i, *part_cnt;                      // split regime: (n_q, n_split, SIMILAR_K_MAX) partial lists, (n_q, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // (n_q, k); score_out / count_out may be null
  float* rows_out; long long ld;                              // poi_similar_rows: rows_out[q * ld + j], ld >= n
  int count_bad;                                              // 0: the caller counts the rejected queries itself (rows + select route)
  int* bad;                                                   // device counter of rejected queries (poi_ctx_take_bad_ids)
};
struct NearestArgs {
  const void* items; int items_f16; int n_item, dim;          // the item rows of the embedding part (null with geo_weight 1)
  const double *coords, *cphi; double geo_weight, scale_km;   // (n_item, 2) lat, lon; cos(lat) (null with geo_weight 0)
  const int* lists; int n, k;                                 // (n, k) listed POIs, -1 fill
  const int *h_off, *h_ids;                                   // CSR of the rows' history POIs, in the order given
  int* pos_out; double* sim_out;                              // (n, k); sim_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_row_inv_norms(const void* x, int x_f16, int n, int dim, double* inv_out, hipStream_t st, Timing* tm);
hipError_t launch_similar(const SimilarArgs& A, hipStream_t st, Timing* tm);         // the fused walk (+ the slices' merge)
hipError_t launch_similar_rows(const SimilarArgs& A, hipStream_t st, Timing* tm);    // the store epilogue
// after poi_topk_select over rows_out: count_out loses the query's own row, a rejected query is counted once and lists nothing
hipError_t launch_similar_fix_counts(const SimilarArgs& A, hipStream_t st);
hipError_t launch_similar_nearest(const NearestArgs& A, hipStream_t st, Timing* tm);

// Route recommendation (route.hip): one beam-search step - per row the best b candidates and the normaliser over all POIs; the merge
#define ROUTE_B_MAX 8                       // beam width: list length, and parents x b <= 64 proposals meet in one wave
#define ROUTE_T_MAX 16                      // steps: the longest path a row may carry
#define ROUTE_SPLIT_LIMIT 64                // workgroups the item range of a 32-row tile may be split over
#define ROUTE_NWAVE 4                       // waves of a workgroup (POI_NWAVE): the item ranges of a tile are n_split * ROUTE_NWAVE
#define ROUTE_LSE_TILES 16                  // 32-item tiles per ITEM BLOCK of the normaliser (512 POIs): the unit of its summation order
struct RouteArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, b;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int* path; int path_stride, path_len;                 // (n, path_stride): path_len ids per row that leave the candidates
  const int *ex_off, *ex; int rows_per_list;                  // exclusion lists (ascending ids), list row / rows_per_list; or both null
  const int* live;                                            // (n) 0: the row is dead and costs nothing; null: every row is live
  int n_split, finish, n_blk;                                 // workgroups per 32-row tile; 1: the tile path (n_split 1) finishes its rows itself; item blocks
  float* part_s; int* part_i;                                 // (rows padded to 32, 4 n_split, ROUTE_B_MAX) partial lists
  double* part_lse;                                           // (rows padded to 32, n_blk, 2): max and rescaled float64 sum of every item block
  int *row_st, *row_cnt;                                      // (rows padded to 32): 0 dead, 1 live, 2 rejected; |C(r)|
  int* idx_out; float* score_out; double* lse_out; int* count_out;      // count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
struct RouteMergeArgs {
  const int* idx; const float* score; const double* lse;      // the expand outputs of n_slot * n_par rows
  const double* total_in; const int* n_live;                  // (n_slot, n_par); (n_slot) live parents (a prefix), or null: all
  int n_slot, n_par, b;
  int *parent_out, *poi_out; double *total_out, *steplp_out; int* nlive_out;      // (n_slot, b); steplp_out / nlive_out may be null
};
hipError_t launch_route_expand(const RouteArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_route_merge(const RouteMergeArgs& A, hipStream_t st, Timing* tm);

// Diversified recommendation (diverse.hip): a pool of the best <= 64 candidates per row, and its MMR re-ranking
#define DIVERSE_POOL_MAX 64                 // pool length (one wave: lane i owns pool position i)
#define DIVERSE_K_MAX 32                    // re-ranked list length
#define DIVERSE_SPLIT_LIMIT 64              // workgroups the item range of a 32-row tile may be split over
#define DIVERSE_NDIST_MAX 4096              // distance bins whose thresholds fit the pool kernel's LDS beside its lists
struct DiverseArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k;                                      // k: the pool length
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  int n_split;                                                // item slices, one workgroup each per 32-row tile (1 on the tile path)
  float* part_s; int *part_i, *part_cnt;                      // split path: (n, n_split, DIVERSE_POOL_MAX) partial lists, (n, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // (n, k) pool ids / scores; count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
struct RerankArgs {
  const int* pool_idx; const float* pool_score; int n, pool;  // (n, pool): position i = the i-th best, -1 ends a row's pool
  const void* items; int items_f16; int n_item, dim;          // the item rows of the embedding part (null with geo_weight 1)
  const double *coords, *cphi;                                // (n_item, 2) lat, lon; cos(lat) (null with geo_weight 0)
  int k; double trade, geo_weight, scale_km;
  int* idx_out; float* score_out; int* pos_out; double* obj_out;      // (n, k); all but idx_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_diverse_pool(DiverseArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_diverse_rerank(const RerankArgs& A, hipStream_t st, Timing* tm);

// Candidate generation (select.hip): explicit score rows from the tile walk, and the exact top-K of score rows for K up to 4096
#define SELECT_K_MAX 4096                   // list length: the sort's 4096 x 8 bytes fit one workgroup's LDS
#define SELECT_SPLIT_LIMIT 64               // slices a row's id range may be cut into
#define SELECT_BINS 2048                    // histogram bins per row (digits of 11 / 11 / 10 bits)
#define SELECT_STATE_INTS 8                 // per-row state between the kernels
#define SELECT_ROWS_MAX 4096                // rows one launch sequence takes (bounds the histogram / candidate workspace)
struct ScoreRowsArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *ex_off, *ex; int* bad;                           // (the operand block's members: not read)
  int n_split;                                                // item ranges (one per wave) of a 32-row tile
  float* out; long long ld;                                   // out[r * ld + j], ld >= n_item
};
struct SelectArgs {
  const float* scores; long long ld; int n, n_item, k;        // (n, ld) float32 score rows, the first n_item of each row are read
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  int n_split;                                                // slices of a row's id range, a workgroup each
  int* hist; int* state; unsigned long long* cand;            // workspace: (n, SELECT_BINS), (n, SELECT_STATE_INTS), (n, k)
  int* idx_out; float* score_out; int* count_out;             // (n, k); score_out / count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_score_rows(const ScoreRowsArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_select(const SelectArgs& A, hipStream_t st, Timing* tm);

// Re-ranking (rerank.hip): the scores of explicit candidate lists, and the best k of every list under explicit (blended) scores
#define RERANK_CHUNK 256                    // entries of a ragged row one workgroup scores at a time (poi_score_lists_chunk)
#define RERANK_LEN_MAX 4096                 // list length / k of the sort: 4096 x 12 bytes fit one workgroup's LDS
#define RERANK_SORT_BLOCK 1024              // threads of the sort's workgroup at lists beyond 2048 entries
struct ScoreListsArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null
  const int *ex_off, *ex; int* bad;                           // (ex_off / ex: the operand block's members, not read); bad: device counter of rejected rows
  const int *cand_off, *cand; int n_cand;                     // ragged: row r owns cand[cand_off[r] .. cand_off[r + 1]); cand_off null: one list for all rows
  int* flag;                                                  // workspace: (n) ragged / (1) shared, 1 = rejected
  int n_split;                                                // ragged: workgroups per row (gridDim.y); shared: list ranges (one per wave) of a 32-row tile
  float* out;                                                 // ragged: (n_cand), parallel to cand; shared: (n, n_cand)
};
struct RerankListsArgs {
  const int *cand_off, *cand; int n, n_cand;                  // the lists, as above
  const float *score, *prior; double w_score, w_prior;        // parallel to cand (ragged) / (n, n_cand) (shared); prior may be null
  const int* flag;                                            // rows the scoring stage of poi_rerank has rejected and counted (not counted again), or null
  int k, p_max;                                               // p_max: the power of two the longest admissible list sorts in
  int* idx_out; float* score_out; int* pos_out; int* count_out;      // (n, k), (n); all but idx_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
hipError_t launch_score_lists(const ScoreListsArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_rerank_lists(const RerankListsArgs& A, hipStream_t st, Timing* tm);

// Filtered recommendation (filter.hip): pass bitmaps of attribute predicates, and the top-K among the POIs whose bit is set
#define FILTER_K_MAX NEAR_K_MAX             // list length (one half wave)
#define FILTER_SPLIT_LIMIT 64               // slices a row's (a 32-row tile's) item range may be cut into
#define FILTER_NCAT_MAX 4096                // categories: the predicate's list is a bit set of this many bits in LDS
#define FILTER_NDIST_MAX 4096               // distance bins whose thresholds fit the walk kernel's LDS beside its lists
struct FilterBuildArgs {
  const int* cat; const unsigned* flags; int n_item, n_cat;   // per POI; either may be null (flags: all-zero words)
  const int *pc_off, *pc; const unsigned *need, *any, *forbid; int n_pred;      // predicate q: categories pc[pc_off[q] .. pc_off[q + 1]) (empty: any), flag words
  unsigned* bits; long long ldw; int* count;                  // (n_pred, ldw) words, bit j & 31 of word j >> 5; (n_pred) popcounts or null
  int* bad;                                                   // device counter: POIs whose category lies outside [0, n_cat) (poi_ctx_take_bad_ids)
};
struct FilterArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null; last_poi = the anchor (null: none)
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  const unsigned* bits; long long ldw; int n_pred; const int* pred;             // pass bitmaps; per-row predicate (null: predicate 0)
  const int* order; double c_r, band_deg;                     // gather path: latitude order, radius (c_r = +inf: none), band half-width
  int n_split;                                                // slices (1 on the tile / row path)
  float* part_s; int *part_i, *part_cnt;                      // split path: (n, n_split, FILTER_K_MAX) partial lists, (n, n_split) counts
  int* idx_out; float* score_out; int* count_out;             // (n, k); score_out / count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
struct FilterScoresArgs {
  const float* scores; long long ld; int n, n_item, k;        // (n, ld) float32 score rows, the first n_item of each row are read
  const int *ex_off, *ex;
  const unsigned* bits; long long ldw; int n_pred; const int* pred;
  int n_split;                                                // (1: list_emit's member)
  float* part_s; int *part_i, *part_cnt;                      // (null: list_emit's members)
  int* idx_out; float* score_out; int* count_out;
  int* bad;
};
hipError_t launch_filter_build(const FilterBuildArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_filter_walk(FilterArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_filter_gather(FilterArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_filter_scores(const FilterScoresArgs& A, hipStream_t st, Timing* tm);

// Capped recommendation (capped.hip): the top-K with at most `per` POIs of one label
#define CAPPED_K_MAX 32                     // list length (one half wave)
#define CAPPED_PER_MAX 32                   // the largest cap; fill tables hold the caps 0 .. CAPPED_PER_MAX
#define CAPPED_FILL_LD (CAPPED_PER_MAX + 1) // ints per predicate of a fill table
#define CAPPED_SPLIT_LIMIT 64               // slices a 32-row tile's item range may be cut into
#define CAPPED_NDIST_MAX 4096               // distance bins whose thresholds fit the walk kernel's LDS beside its lists
struct LabelsBuildArgs {
  const int* labels; int n_item, n_label;                     // per POI: >= 0 a group, < 0 unlabelled; >= n_label: a bad id, entered as unlabelled
  const unsigned* bits; long long ldw; int n_pred;            // pass bitmaps, or null (one row: every POI passes)
  int *hist, *unl;                                            // workspace: (rows, n_label) passing POIs per label, (rows) unlabelled ones; unl = hist + rows * n_label
  int* count; int* fill;                                      // (n_label) POIs per label or null; (rows, CAPPED_FILL_LD)
  int* bad;                                                   // device counter: POIs whose label is >= n_label (poi_ctx_take_bad_ids)
};
struct CappedArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim, k;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null; last_poi = the anchor (null: none)
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  const int* labels; int per; const int* fill;                // labels (n_item); the cap; fill table (n_pred or 1, CAPPED_FILL_LD) or null
  const unsigned* bits; long long ldw; int n_pred; const int* pred;             // pass bitmaps or null (then n_pred = 1); per-row predicate (null: predicate 0)
  int n_split;                                                // slices (1 in the block regime)
  float* part_s; int *part_i, *part_cnt;                      // split regime: (n, n_split, CAPPED_K_MAX) partial lists, (n, n_split) counts
  int* idx_out; float* score_out; int* label_out; int* count_out;               // (n, k); score_out / label_out / count_out may be null
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
struct CappedScoresArgs {
  const float* scores; long long ld; int n, n_item, k;        // (n, ld) float32 score rows, the first n_item of each row are read
  const int *ex_off, *ex;
  const int* labels; int per; const int* fill;
  const unsigned* bits; long long ldw; int n_pred; const int* pred;
  int* idx_out; float* score_out; int* label_out; int* count_out;
  int* bad;
};
hipError_t launch_labels_build(const LabelsBuildArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_capped_walk(const CappedArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_capped_scores(const CappedScoresArgs& A, hipStream_t st, Timing* tm);

// Label recommendation (labels.hip): per row and label the softmax mass, the best POI and the number of the candidates
#define LABELS_K_MAX 32                     // labels a top-K call lists per row
#define LABELS_SPLIT_LIMIT 64               // slices a 32-row tile's item range may be cut into
#define LABELS_NDIST_MAX 4096               // distance bins whose thresholds fit the walk kernel's LDS beside its accumulators
#define LABELS_LDS_KB_MAX 120               // the most LDS (KiB) the accumulators of a workgroup may take (option "labels_lds_kb")
#define LABELS_ROW_BYTES 20                 // accumulator bytes per (row, bucket): 64-bit mass, 64-bit best key, 32-bit count
#define LABELS_Q_BITS 36                    // q = round(exp(s - M) 2^36)
#define LABELS_BY_MASS 0
#define LABELS_BY_MAX 1
struct LabelsAcc {                                            // context workspace of one chunk of rows, zero before the walk
  unsigned long long *mass, *best; unsigned* cnt;             // (rows, n_label + 1): bucket n_label holds the unlabelled POIs
  unsigned* mkey; int* status;                                // (rows): f2ord(M(r)), 0 = none; 1 = the row was rejected
};
struct LabelsArgs {
  const float* users; const void* items; int items_f16;      // (n, dim) float32; (n_item [+ 1], dim) float32 or IEEE half
  int n, n_item, dim;
  const float *wd, *sts; const double *coords, *cphi, *thr; const int* last_poi; int n_dist; float bin_scale;      // distance term, or wd null; last_poi = the anchor (null: none)
  const int *ex_off, *ex;                                     // per-row exclusion lists (ascending ids), or both null
  const int* labels; int n_label;                             // labels (n_item): [0, n_label) a label, anything else unlabelled
  int n_split;                                                // slices (1 in the tile regime)
  int lds_home;                                               // the accumulators of a workgroup live in LDS and are flushed once (else: atomics on acc)
  LabelsAcc acc;
  int* bad;                                                   // device counter of rejected rows (poi_ctx_take_bad_ids)
};
struct LabelsScoresArgs {
  const float* scores; long long ld; int n, n_item;           // (n, ld) float32 score rows, the first n_item of each row are read
  const int *ex_off, *ex;
  const int* labels; int n_label;
  int lds_home;
  LabelsAcc acc;
  int* bad;
};
struct LabelsFinishArgs {
  int n, n_label, k, by;                                      // k = 0: no top-K part
  LabelsAcc acc;
  unsigned long long* mass_out; int* best_id_out; float* best_score_out; int* count_out;      // dense (n, n_label + 1), each may be null
  float* m_out; double* lognorm_out;                          // (n), may be null
  int* label_out; double* logp_out; int* top_id_out; float* top_score_out;      // (n, k); all but label_out may be null
  int* n_listed_out; double* rest_logp_out;                   // (n), may be null
};
hipError_t launch_labels_max(const LabelsArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_labels_walk(const LabelsArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_labels_scores(const LabelsScoresArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_labels_finish(const LabelsFinishArgs& A, hipStream_t st, Timing* tm);
size_t labels_lds_bytes(int rows, int n_label);              // LDS the accumulators of `rows` rows take

// Fold-in of new users for the factorisation family (foldin.hip)
#define FOLDIN_USERS_PER_WAVE 4             // one 16-lane DPP row per user
struct FoldinArgs {
  const void* items; int items_f16;                           // (n_item + 1, dim) float32 or IEEE half
  int n, n_item, dim, epochs;
  const int *off, *p, *q; long long q_epoch_stride;           // history CSR (n + 1), positives, negatives of epoch e at q + e * q_epoch_stride
  float alpha, lambda;
  const float* w0; float* w_out; float* loss_out;             // (n, dim) or null; (n, dim), may alias w0; (n, epochs) or null
  int* bad;                                                   // device counter of rejected users (poi_ctx_take_bad_ids)
};
hipError_t launch_foldin(const FoldinArgs& A, hipStream_t st, Timing* tm);

// Fold-in of new users for the successive-POI models (foldin_seq.hip): the per-step scalars a / c, then the generalised chain
#define FOLDIN_FORM_DOT 0                   // x = w . d + c                                   (FPMC-LR's ui against iu)
#define FOLDIN_FORM_METRIC 1                // x = a (|w - y_q|^2 - |w - y_p|^2) + c           (PRME's du against dp)
struct FoldinTermsArgs {
  const float *tab_pq, *tab_prev;                             // FPMC-LR: ia, ai;  PRME: ds, ds   (n_item + 1, dim) float32
  int n, n_item, dim, n_epoch;                                // n_epoch: epochs with their own negatives (1 when q_epoch_stride = 0)
  long long total;                                            // check-ins of the call (length of p)
  const int *off, *p, *q; long long q_epoch_stride;
  const int* gap; const double *dist, *cordi; int thd; float cw;      // PRME only; dist or cordi
  double *a_out, *c_out;                                      // a_out (total), PRME only; c_out at the stride of q
};
hipError_t launch_foldin_terms(const FoldinTermsArgs& A, bool prme, int num_cu, hipStream_t st, Timing* tm);
struct FoldinPairArgs {
  const float* items;                                         // (n_item + 1, dim) float32
  int n, n_item, dim, epochs, form, first;
  const int *off, *p, *q; long long q_epoch_stride;
  const double *a, *c; long long c_epoch_stride;              // per-position weight (metric form) and offset, or null (1 and 0)
  const double* dummy;                                        // 8 readable bytes: where the loads of absent a / c and of steps past the end go
  float alpha, lambda;
  const float* w0; float* w_out; float* loss_out;
  int* bad;
};
hipError_t launch_foldin_pair(const FoldinPairArgs& A, hipStream_t st, Timing* tm);

// Fold-in of new users for POI2Vec (foldin_p2v.hip): the xu[u] part of the step against the frozen wl, one softmax pass per epoch
#define P2V_FOLD_SPAN 256                   // items per partial: a user's (max, sum, weighted row sum) partials are merged in span order
#define P2V_FOLD_USERS 64                   // users per workgroup of the pass kernel (four 16-user MFMA tiles share a staged item tile)
struct FoldP2vArgs {
  const float* wl;                                            // (>= n_item, dim) float32: the softmax runs over rows 0 .. n_item - 1
  int n, n_item, dim, epochs, n_span, epoch;                  // n_span = ceil(n_item / P2V_FOLD_SPAN); epoch: set per launch
  const int *off, *tgt;                                       // history CSR (n + 1), targets
  float alpha, lambda;
  const float* w0; float* w_out; float* loss_out;             // (n, dim) or null; (n, dim), may alias w0; (n, epochs) or null
  double *w, *tbar, *part; int* flag;                         // scratch: (n, dim) running rows, (n, dim) mean target rows,
                                                              // (n, n_span, dim + 2) partials; per user 0 = live, 1 = bad, 2 = nothing to do
  int* bad;                                                   // device counter of rejected users (poi_ctx_take_bad_ids)
};
size_t foldin_p2v_lds(int dim);
hipError_t launch_foldin_p2v(FoldP2vArgs& A, hipStream_t st, Timing* tm);

// scoring / top-K
struct ScoreArgs {
  const float *users, *items; int items_f16;      // items: float32, or IEEE half when items_f16
  float4* items_packed;     // MFMA B-fragment order (large-n kernel), ctx scratch
  int n, n_item, dim;
  const float *wd, *prob;
  // distance term through the resident bin matrix (ulptai_kernel layout) instead of `prob`:
  // score += wd * (bin < n_dist ? sts[user][bin] : 0)
  const void* ulptai; int bin_bytes; const float* sts; int n_dist;
  // ... or with the bins computed on the fly from the coordinates (no U x N matrix at all): geo != 0
  int geo; const double *coords, *cphi, *thr; const int* last_poi; double dd;
  float* scores;            // (n, n_item) or null
  int k;                    // 0 = no top-K
  int n_split;              // item splits for the fused top-K
  float* cand_score; int* cand_idx;   // (n_split, n_pad, k) partial top-K lists
  int dbg;                  // tuning switch (POI_SCORE_DBG), 0 in production
  int max_stride;           // score_filter_kernel<MAXP>: every max_stride-th item tile
  unsigned* gbound;         // (n_pad) per-user lower bound of the K-th best score shared by all item ranges
  int seeded;               // gbound starts from the caller's seed items' scores (topk_seed_kernel), not from zero
  int* idx_out; float* score_out;
  // two-stage path (score_filter.hip): half-precision item fragments + per-item norms of the bound, per-user survivor lists, and the
  // per-user-tile overflow flags; the one-stage kernels and the merge skip every tile whose flag is clear when tile_flag is set
  const uint4* items_packed16; const float2* inorm;
  int* surv_cnt; int* surv_idx; float* surv_sc; int* tile_flag;
  // item-stationary GEO filter (score_filter_items_kernel): the users' half fragments, per-user bound terms and last-POI coordinates
  // (ctx scratch; users_packed16 == nullptr: the user-stationary filter), and the CU count for its persistent grid
  uint4* users_packed16; float4* ubound; double* ugeo; int n_cu;
  int bins_ntile;           // item tiles per user-tile row of the bin matrix when the call scores only a PREFIX of the item table (0: = tiles of n_item)
};
// two-stage path (score_filter.hip); every grid, LDS size and kernel choice comes from the call's plan (score_plan.h)
hipError_t launch_score_two_stage(const ScoreArgs& A, const ScorePlan& P, hipStream_t st, Timing* tm);
hipError_t launch_score_maxpass(const ScoreArgs& A, const ScorePlan& P, hipStream_t st, Timing* tm);      // unseeded calls: thresholds from block maxima of the f16 lower bounds
hipError_t launch_topk_bound(const float* score_k, int n, int k, unsigned* gbound, hipStream_t st);
hipError_t launch_ulptai(const double* coords, const double* cphi, const double* thr, const int* last_poi, int n, int n_item,
                         int n_dist, double dd, void* out, int bin_bytes, hipStream_t st);
hipError_t launch_score(const ScoreArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_score_packed(const ScoreArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_topk_seed(const ScoreArgs& A, const int* seed, int k_seed, hipStream_t st);
hipError_t launch_score_geo_stream(const ScoreArgs& A, hipStream_t st, Timing* tm);
hipError_t launch_topk_merge(const ScoreArgs& A, int n_lists, int n_pad, hipStream_t st);
hipError_t launch_topk_rows(const float* scores, int n, int n_item, int k, int* idx_out, float* score_out, hipStream_t st);

// misc
hipError_t launch_auc(const float* users, const float* items, int items_f16, int n, int dim, const int* tp, const int* tq,
                      const int* tm, int len, uint8_t* out, hipStream_t st);
hipError_t launch_sumsq_f16(const void* x, int64_t n, double* out, hipStream_t st);
hipError_t launch_sumsq(const float* x, int64_t n, double* out, hipStream_t st);
hipError_t launch_dist_prob(const double* coords, const double* cphi, const double* thr, const int* last_poi, const float* sts,
                            int n, int n_item, int n_dist, double dd, float* prob, hipStream_t st);
hipError_t launch_rank_metrics(const int* ranks, int n, int K, const int* tes_p, const int* tes_mask, int len_tes, const int* at_nums,
                               int n_at, double* acc, hipStream_t st);
hipError_t launch_sample_neg(const int* off, const int* p, int n_user, int n_item, const int* tes_p, const int* tes_mask, int len_tes,
                             unsigned long long seed, int* q_out, int* tes_q_out, hipStream_t st);
hipError_t launch_neg_dist(const int* off, const int* p, const int* q, int n_user, const double* coords, const double* cphi,
                           const double* thr, int n_dist, double dd, int* dq, hipStream_t st);
hipError_t launch_delta_make(const float* cur, const float* base, float* delta, int64_t n, hipStream_t st);
hipError_t launch_delta_apply(float* cur, const float* base, const float* dsum, int64_t n, hipStream_t st);
hipError_t launch_selftest(float* buf, int* fail, hipStream_t st);

}  // namespace poi
