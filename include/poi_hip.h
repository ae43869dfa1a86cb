/*
 * poi_hip.h - C-ABI of libpoi_hip.so: the MI355X (gfx950) implementation of the next-POI hot path
 * of tangrizzly/Point-of-Interest-Recommendation.
 *
 * The reference has no FFI of its own: the hot path sits behind the duck-typed Theano model object
 * that prog_bpr_gru_spatial.py and public/Valuate.py call.  Each entry point below
 * names the reference method whose arithmetic it replaces (file:line relative to /root/reference);
 * the Python classes in point-of-interest-recommendation_amd/models.py mirror those methods and
 * reach this library through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (e.g. torch.Tensor.data_ptr()) unless its name ends in _host.
 *    Nothing is allocated for the caller; scratch memory is owned by the poi_ctx.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue work;
 *    the caller synchronises (outputs are device buffers).
 *  - Return value: 0 on success, a negative POI_E* code otherwise; poi_last_error() returns the text.
 *  - Index data is CSR-packed, never padded on the device: sequence u occupies positions
 *    off[u] .. off[u+1]-1 of the flat int32 arrays p/q/dp/dq.  The reference pads every user to
 *    len_max (public/Load_Data_by_length.py:115-124); the only arithmetic effect of the padding -
 *    the L2 decay of the padding rows lt[n_item] / di[n_dist] (public/GRU_Spatial.py:202-203) - is
 *    reproduced analytically from `len_max`.
 *  - Table element type: float32; the POI table may be stored as IEEE half (poi_ctx_register_f16).  All arithmetic is float32
 *    (reference: float64).
 *
 * Batch semantics (n_seq > 1, "throughput mode"; n_seq == 1 is exactly the reference step):
 *    every sequence's reference update is evaluated at the launch-entry parameter values; each
 *    parameter row then moves by the MEAN of the updates of the sequences that touch it (dense
 *    tensors are touched by all n_seq sequences).  See DESIGN.md "Batch semantics".
 *    poi_ctx_set_batch_cap(cap) generalises the rule: a row touched by k sequences moves by
 *    min(k, cap) / k times the SUM of their updates - cap = 1 (default) is the mean, cap = infinity the plain sum,
 *    i.e. to first order in alpha what k sequential reference steps would do; in between, up to `cap` updates
 *    count in full and hot rows (popular POIs, distance bins, the dense tensors) are averaged down to `cap`.
 */
#ifndef POI_HIP_H
#define POI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 4): poi_sync_buffer no longer carries the deltas of POI_F16 segments - they travel in poi_sync_buffer16, and poi_sync_apply
 * refuses to combine half segments whose buffer the caller never asked for; new entry points since 2: poi_sync_buffer16,
 * poi_ctx_set_split_products / _small_launch / _one_sequence_path / _regroup_min / _f16_rounding / _topk_filter(_stats), poi_ctx_set_exact_forward. */
/* 4 (round 4): new entry point poi_ctx_set_option. */
/* 5 (round 5): new entry point poi_comm_available; poi_bpr_step's snapshot mode is sorted and atomic-free and accepts a half POI table; the exact
 * forward pass covers dim 256 (config X); option "hot_bins". */
/* 7: FPMC-LR - new entry points poi_fpmc_neighbor_counts / _fill, poi_fpmc_sample_negatives, poi_fpmc_step (existing entries unchanged). */
/* 8: PRME - new entry points poi_prme_step, poi_prme_score_all, poi_prme_score_topk and poi_prme_params (existing entries unchanged). */
/* 9: new entry point poi_ctx_last_plan (existing entries unchanged). */
/* additive to 9: GeoIE - new entry points poi_geoie_step, poi_geoie_pair_distances, poi_geoie_user_vectors and poi_geoie_params (existing
 * entries unchanged). */
/* additive to 9: POI2Vec - new entry points poi_poi2vec_step, poi_poi2vec_scores, poi_poi2vec_topk and poi_poi2vec_params (existing
 * entries unchanged). */
/* additive to 9: mini-batch Lstm / Rnn - new entry points poi_cell_step, poi_cell_predict and poi_cell_params, option "cell_grid", plan
 * keys for them (existing entries unchanged). */
/* additive to 9: online sessions - new entry points poi_session_advance and poi_session_sts, option "session_tile_min", plan keys
 * "session_path" / "session_tiles" / "session_tile_min" (existing entries unchanged). */
/* additive to 9: VBPR - new entry points poi_vbpr_step, poi_vbpr_items, poi_vbpr_users and poi_vbpr_params, option "vbpr_grid" (existing
 * entries unchanged). */
/* additive to 9: restricted recommendation - new entry point poi_score_topk_near (public/Valuate.py:132-146 over the candidate sets of
 * public/Load_Data_fpmc_lr.py:114-143), options "near_split_max" / "near_grid", plan keys "near_path" / "near_splits" / "near_split_max"
 * (existing entries unchanged). */
/* additive to 9: exact target ranks - new entry points poi_score_rank and poi_rank_scores, option "rank_grid", plan key "rank_splits",
 * timing names "score_rank" / "rank_scores" (existing entries unchanged). */
/* additive to 9: fold-in for the factorisation family - new entry point poi_foldin_bpr, timing name "foldin"; no new option or plan key
 * (existing entries unchanged). */
/* additive to 9: fold-in for the successive-POI models - new entry points poi_foldin_terms_fpmc, poi_foldin_terms_prme and poi_foldin_pair,
 * timing names "foldin_terms" and "foldin_pair"; no new option or plan key (existing entries, poi_foldin_bpr included, unchanged). */
/* additive to 9: online sessions of Lstm / Rnn / CA-RNN - new entry points poi_session_cell_advance and poi_session_carnn_advance,
 * timing names "session_cell_advance" / "session_carnn_advance"; they read the option "session_tile_min" and write the plan keys
 * "session_path" / "session_tiles" / "session_tile_min" as poi_session_advance does (existing entries unchanged). */
/* additive to 9: GeoIE scoring under the trained geo-influence law - new entry points poi_geoie_score_all_geo and poi_geoie_score_topk_geo,
 * option "geoie_score_span", plan keys "geoie_score_span" / "geoie_score_splits", timing names "geoie_score_geo" / "geoie_topk_geo" (existing
 * entries unchanged). */
/* additive to 9: fold-in for POI2Vec - new entry points poi_foldin_p2v, poi_foldin_p2v_span and poi_poi2vec_topk_ex, timing names
 * "foldin_p2v_prep" / "foldin_p2v_pass" / "foldin_p2v_upd"; no new option or plan key (existing entries, poi_poi2vec_scores / _topk
 * included, unchanged). */
/* additive to 9: group recommendation - new entry points poi_group_topk and poi_group_topk_scores, options "group_split_max" / "group_grid",
 * plan keys "group_path" / "group_splits" / "group_split_max", timing names "group_topk" / "group_topk_scores" (existing entries unchanged). */
/* additive to 9: route recommendation - new entry points poi_route_expand and poi_route_merge, options "route_split_max" / "route_grid",
 * plan keys "route_path" / "route_splits", timing names "route_expand" / "route_merge" (existing entries unchanged). */
/* additive to 9: diversified recommendation - new entry points poi_diverse_pool, poi_diverse_rerank and poi_diverse_topk, options
 * "diverse_split_max" / "diverse_grid", plan keys "diverse_path" / "diverse_splits" / "diverse_split_max", timing names "diverse_pool" /
 * "diverse_rerank" (existing entries unchanged). */
/* additive to 9: candidate generation - new entry points poi_score_rows, poi_topk_select and poi_score_candidates, options
 * "select_split_max" / "select_grid" / "select_chunk_mb", plan keys "select_rows_per_chunk" / "select_chunks" / "select_path" /
 * "select_splits", timing names "score_rows" / "topk_select" / "score_candidates" (existing entries unchanged). */
/* additive to 9: filtered recommendation - new entry points poi_filter_build, poi_score_topk_filtered and poi_topk_filtered_scores, the
 * POI_FILTER_* path constants, options "filter_split_max" / "filter_grid" / "filter_gather_cost", plan keys "filter_path" /
 * "filter_splits" / "filter_split_max", timing names "filter_build" / "score_topk_filtered" / "topk_filtered_scores" (existing entries
 * unchanged). */
/* additive to 9: audience recommendation - new entry points poi_score_audience and poi_audience_rows, options "audience_split_max" /
 * "audience_grid", plan keys "audience_path" / "audience_splits" / "audience_split_max", timing names "score_audience" (with
 * "audience_walk" / "audience_merge" inside it) / "audience_rows" (existing entries unchanged). */
/* additive to 9: similar POIs and users - new entry points poi_row_inv_norms, poi_similar_topk, poi_similar_rows and
 * poi_similar_nearest, options "similar_split_max" / "similar_grid" / "similar_rows_max", plan keys "similar_path" / "similar_splits" /
 * "similar_split_max", timing names "similar_topk" (with "similar_norms" / "similar_walk" / "similar_merge" or "similar_rows" /
 * "topk_select" inside it) / "similar_rows" / "similar_nearest" (existing entries unchanged). */
/* additive to 9: capped recommendation - new entry points poi_labels_build, poi_score_topk_capped and poi_topk_capped_scores, options
 * "capped_split_max" / "capped_grid" / "capped_hist_kb", plan keys "capped_splits" / "capped_split_max", timing names "labels_build" / "score_topk_capped"
 * (with "capped_walk" / "capped_merge" inside it) / "topk_capped_scores" (existing entries unchanged). */
/* additive to 9: re-ranking - new entry points poi_score_lists, poi_rerank_lists and poi_rerank (and poi_score_lists_chunk), plan key
 * "lists_path", timing names "score_lists" / "rerank_lists" / "rerank"; no new option (existing entries unchanged). */
/* additive to 9: label recommendation - new entry points poi_score_labels, poi_score_topk_labels and poi_labels_scores, options
 * "labels_split_max" / "labels_grid" / "labels_lds_kb" / "labels_ws_kb", plan keys "labels_splits" / "labels_split_max" / "labels_home" /
 * "labels_chunks" / "labels_rows_per_chunk", timing names "score_labels" / "score_topk_labels" / "labels_scores_call" (with "labels_max" /
 * "labels_walk" or "labels_scores", and "labels_finish" inside them) (existing entries unchanged). */
/* additive to 9: leave-one-out attribution - new entry point poi_explain_loo, option "explain_start", plan keys "explain_columns" /
 * "explain_tiles" / "explain_start", timing names "explain_base" / "explain_walk" (existing entries unchanged). */
#define POI_ABI_VERSION 9

enum {
  POI_OK = 0,
  POI_EINVAL = -1,   /* bad argument (NULL pointer, D % 4 != 0, n < 0, ...) */
  POI_ENOMEM = -2,   /* scratch allocation failed */
  POI_EHIP = -3,     /* a HIP runtime call failed */
  POI_ENOTSUP = -4   /* configuration not supported by this build */
};

/* Table element types.  Every table is float32 unless its buffer has been registered as IEEE half with
 * poi_ctx_register_f16 (config X: "fp16 embeddings"): storage only - all arithmetic stays float32, rows are converted when they are
 * gathered and rounded to nearest-even when they are written back. */
enum { POI_F32 = 0, POI_F16 = 1 };

typedef struct poi_ctx poi_ctx;

/* Parameter block of the recurrent models.
 *   OboSpatialGru (public/GRU_Spatial.py:42-90): all fields; ui is (3, D, 2D).
 *   OboGru        (public/GRU.py:301-311):        di/vs/bs/wd/lw NULL, n_dist 0; ui is (3, D, D).
 * lt (n_item+1, D)  di (n_dist+1, D)  wh (3, D, D)  bi (3, D)  vs (n_dist+1, D)  bs (n_dist+1)
 * wd (1)  lw = loss_weight (2).  h0 is the zero vector (never trained, public/GRU_Spatial.py:80-82). */
typedef struct poi_gru_params {
  float* lt; float* di; float* ui; float* wh; float* bi; float* vs; float* bs; float* wd; float* lw;
  int32_t n_item; int32_t n_dist; int32_t dim;
} poi_gru_params;

/* CSR view of the reference's shared index tables tra_buys_masks / tra_buys_neg_masks /
 * tra_dist_masks / tra_dist_neg_masks / tra_masks (public/GRU.py:50-55, public/GRU_Spatial.py:46-49).
 * dp/dq may be NULL for OboGru.  len_max = padded row length of the reference tables. */
typedef struct poi_seq_tables {
  const int32_t* off; const int32_t* p; const int32_t* q; const int32_t* dp; const int32_t* dq;
  int32_t n_user; int32_t len_max; int32_t max_len; /* max_len = longest real sequence */
} poi_seq_tables;

/* ---- context ------------------------------------------------------------------------------- */
int poi_abi_version(void);
int poi_ctx_create(poi_ctx** out, int device);
int poi_ctx_destroy(poi_ctx* ctx);
const char* poi_last_error(const poi_ctx* ctx);   /* also valid with ctx == NULL (last global error) */
/* number of CUs / name of the device the ctx is bound to (host-side queries) */
int poi_ctx_num_cu(const poi_ctx* ctx);

/* Engine used by poi_spatial_step / poi_gru_step / poi_gru_predict: 0 = auto (tile engine whenever dim is 64, 128 or 256 and
 * n_dist+1 <= 2048 - also for a single sequence, where it is ~5x faster -, per-sequence engine otherwise; beyond 256 bins the
 * head runs bin-chunked with an online softmax and the distance-bin half of the input goes through the GEMMs again),
 * 1 = per-sequence engine, 2 = tile engine whenever supported, 3 = tile engine with the streaming recurrent kernels of
 * dim 256 (32-sequence tiles, weights streamed from L2) also at dim 128 - a testing aid.  Engines 0 - 3 implement the same float32
 * arithmetic (only the summation order differs).
 * 4 = EXACT: float64 arithmetic end to end (exact_engine.hip; the reference's Theano floatX is float64, public/GRU.py:57) - the float32
 * tables are converted when gathered and rounded to nearest once at the write-back, every intermediate (gates, hidden states, softmax,
 * BPTT, dense and sparse gradient sums, the SGD update) is float64, and alpha / lambda are taken as the shortest decimals that round to
 * the given floats (0.01f -> 0.01).  The opt-in mode for BASELINE.json's "weights within 1e-5 after one step" on EVERY row at the full
 * shapes, where float32 BPTT misses it on ~0.1 % of the rows; any dim % 4 == 0 up to 256, <= 4095 bins, float32
 * tables; ~30x slower than the tile engine.  Also settable with POI_ENGINE=seq|tile|exact. */
int poi_ctx_set_engine(poi_ctx* ctx, int engine);
/* hipGraph replay of the tile engine's training launch (poi_spatial_step / poi_gru_step): the ~40 kernels a launch enqueues on two
 * streams are captured once per launch shape (second launch with the same parameters / tables / n / alpha / lambda) and replayed with
 * ONE hipGraphLaunch; the caller's uidx / out pass through context-owned staging buffers, so any uidx / out pointer replays the same
 * graph.  Same kernels, same order, same bits as the eager launch.  Off by default (POI_GRAPH=1 enables): on ROCm 7.0 / MI355X a
 * replay takes exactly as long as the eager launch - the launch is bound by the dependent-dispatch chain on the GPU, not by the host
 * (tools/bench_graph.py).  on = 1 replays launches of min_n <= n <= max_n sequences.  Kernel timing (poi_timing_enable) needs eager launches and switches replay off while it is on.
 * poi_ctx_graph_replays: number of launches served by a replay so far. */
int poi_ctx_set_graph(poi_ctx* ctx, int on, int min_n, int max_n);
int64_t poi_ctx_graph_replays(const poi_ctx* ctx);
/* ABI 6.  Out-of-range ids in poi_bpr_step (the reference - a Theano gather, public/BPR.py:214-218 - raises IndexError): the kernels never touch
 * memory outside the tables; a triple with a user id outside [0, n_user) or a POI id outside [0, n_item] is REJECTED: it adds no gradient, no L2
 * decay and no multiplicity to any row - the rows its valid ids name included - its loss is NaN, and it is counted on the device, once per triple
 * however many of its ids are bad, in both modes.  Removal rule: in snapshot mode the launch equals the launch without its rejected triples, bit
 * for bit (tables and kept losses).  poi_ctx_take_bad_ids synchronises `stream`, returns the count since the last call and clears it - the Python
 * mirror raises IndexError from OboBpr.train / train_batch(sync=True), as the reference does.  ABI 7: poi_fpmc_step counts its rejected
 * transitions (an id outside its table, or i == j) in the same counter, one per transition.  ABI 8: so does poi_prme_step. */
int64_t poi_ctx_take_bad_ids(poi_ctx* ctx, void* stream);
/* ABI 9.  The plan the last poi_spatial_step / poi_gru_step on this context took, one named value at a time:
 * "tile", "one", "rec1", "xrec1", "hyb", "bintab", "ppoi", "listed", "fwd_tab", "xft", "xcomp", "head_split", "efuse",
 * "early_bins", "fork", and "hyb_fwd_seq" / "hyb_fwd_wg" / "hyb_bwd_seq" / "hyb_bwd_wg" (TeArgs.hyb_dev; synchronises the
 * launch stream; -1 when hyb == 0).  POI_EINVAL for an unknown key, or before any training launch.  The flags are host fields set
 * where the launch decides them (a graph replay records the plan of the launch it replays); "tile" == 0: the per-sequence or the exact
 * engine ran and every other flag is 0.  The hyb_* values live in the tile engine's workspace: POI_EINVAL once a later tile-engine
 * launch (poi_gru_predict included) may have reused it.
 * Additive to 9: "cell_kernel" and "cell_grid" - the gate-block count (POI_CELL_RNN / POI_CELL_LSTM) of the recurrent kernel and the
 * workgroups of its persistent grid when the last training launch was a poi_cell_step, 0 otherwise.
 * Additive to 9: "session_path", "session_tiles", "session_tile_min" - written by poi_session_advance (which leaves the other keys as they
 * are and also makes the plan readable).
 * Additive to 9: "near_path", "near_splits", "near_split_max" - written by poi_score_topk_near in the same way.
 * Additive to 9: "rank_splits" - written by poi_score_rank in the same way.
 * Additive to 9: "geoie_score_span", "geoie_score_splits" - written by poi_geoie_score_all_geo / poi_geoie_score_topk_geo in the same way.
 * Additive to 9: "group_path", "group_splits", "group_split_max" - written by poi_group_topk in the same way.
 * Additive to 9: "route_path", "route_splits" - written by poi_route_expand in the same way.
 * Additive to 9: "diverse_path", "diverse_splits", "diverse_split_max" - written by poi_diverse_pool / poi_diverse_topk in the same way.
 * Additive to 9: "select_rows_per_chunk", "select_chunks" - the chunking poi_score_candidates took (rows of score rows held at a time,
 * number of chunks); "select_path", "select_splits" - written by poi_topk_select / poi_score_candidates in the same way.
 * Additive to 9: "xfwd_ids_lds" - 1 when the launch took the table form of the exact forward recurrence with its row ids staged in LDS
 * (option of the same name), 0 with the ids loaded inside the step loop or without the table form; poi_gru_predict records its own value
 * of this one key.
 * Additive to 9: "stream_hints" - 1 when the 16-sequence tiles of the launch's exact forward recurrence stored G, H and RH non-temporally
 * (option of the same name), 0 otherwise.
 * Additive to 9: "filter_path" (1 walk, 2 gather), "filter_splits" (slices, 0 outside the split regime), "filter_split_max" - written
 * by poi_score_topk_filtered.
 * Additive to 9: "audience_path" (0 one workgroup per query block, 1 slices), "audience_splits" (slices, 0 outside the split regime),
 * "audience_split_max" - written by poi_score_audience / poi_audience_rows.
 * Additive to 9: "similar_path" (0 one workgroup per query block, 1 slices, 2 score rows + selection), "similar_splits" (slices of the
 * walk, 0 with one workgroup per query block), "similar_split_max" - written by poi_similar_topk / poi_similar_rows.
 * Additive to 9: "capped_splits" (slices, 0 outside the split regime), "capped_split_max" - written by poi_score_topk_capped.
 * Additive to 9: "lists_path" (0 ragged lists, 1 one shared list) - written by poi_score_lists / poi_rerank.
 * Additive to 9: "labels_splits" (slices, 0 outside the split regime), "labels_split_max", "labels_home" (where the label accumulators of
 * the call lived: 1 the workgroup's LDS, 2 the context's global accumulator), "labels_chunks" / "labels_rows_per_chunk" (the rows went
 * through the accumulator workspace in this many chunks of this many rows) - written by poi_score_labels / poi_score_topk_labels /
 * poi_labels_scores.
 * Additive to 9: "explain_columns" (base + variant columns of the call), "explain_tiles" (16-column workgroups of its two launches),
 * "explain_start" (the start mode in force) - written by poi_explain_loo. */
int poi_ctx_last_plan(poi_ctx* ctx, const char* key, int64_t* value);
/* fp16 POI tables: declare that the device buffer [ptr, ptr + bytes) holds IEEE half elements.  From then on every entry point that is
 * handed a pointer INSIDE a registered buffer as its POI table (`lt` of poi_gru_params for poi_spatial_step / poi_gru_step /
 * poi_gru_predict; `items` of poi_score_all / poi_score_topk* / poi_auc_preference; `x` of poi_sumsq) reads / writes it as half.
 * Supported by the tile engine (dim 64 / 128 / 256) and the scoring / AUC / L2 kernels; the per-sequence engine, BPR-MF and CA-RNN
 * return POI_ENOTSUP for a half table.  poi_ctx_unregister_f16(ptr) forgets the buffer (call it before freeing). */
int poi_ctx_register_f16(poi_ctx* ctx, const void* ptr, int64_t bytes);
int poi_ctx_unregister_f16(poi_ctx* ctx, const void* ptr);
/* Rounding of the sparse SGD write-back into a HALF POI table (poi_spatial_step / poi_gru_step, tile engine): mode 0 = round to nearest
 * even (default; an update below half an fp16 ulp of the element - e.g. the whole L2 decay alpha lambda |x| of a row without a loss
 * gradient - is lost), mode 1 = STOCHASTIC rounding: the element rounds up with probability (value - floor) / ulp, so the expected stored
 * value is the float32 result and sub-ulp updates (the decay the reference applies at every step, public/GRU_Spatial.py:202-209) act in
 * expectation.  Counter-based: the same seed and launch sequence reproduce the same tables. */
int poi_ctx_set_f16_rounding(poi_ctx* ctx, int mode, uint32_t seed);
/* Arithmetic of the recurrent kernels of the tile engine (dim 64 / 128: register-resident weights; dim 256: the streaming kernels, whose
 * weight planes are streamed from L2) (h_{t-1} . wh^T forward, da . wh backward - the contractions
 * of public/GRU_Spatial.py:127-171 that sit on the per-step dependency chain).  on = 1 (default): SPLIT products - both operands as three
 * bf16 planes (x = x1 + x2 + x3 to 2^-27), the six partial products down to 2^-16 on v_mfma_f32_16x16x32_bf16 with float32 accumulation:
 * the float32-input MFMA runs at the vector rate on gfx950, this form at 2.7x less matrix time and a product error of 2^-25 (below the
 * float32 accumulation noise; the timed Gowalla launch measures 4.7e-6 against the float64 oracle, 5.7e-6 with on = 0).
 * The switch also covers the forward table of large launches (every POI row times the POI half of ui: te_ptab_s3, dim 128) and
 * the softmax head of configurations with more than 256 distance bins (the reference's dd = 25 m: 1520 bins,
 * public/GRU_Spatial.py:247): logits and d h of the chunked head on the same split products (te_head_big3) instead of float32-input MFMAs.
 * on = 0: float32-input v_mfma_f32_16x16x4_f32 (rounds 1 - 2).  Environment override at context creation: POI_TE_SPLIT=0|1. */
int poi_ctx_set_split_products(poi_ctx* ctx, int on);
/* Exact forward pass of the tile engine's training launches AND of poi_gru_predict (dims 64 / 128 / 256; default on).  The reference computes in float64 (Theano
 * floatX: public/GRU.py:57, public/GRU_Spatial.py:52) and with its uniform(-0.5, 0.5) init the forward recurrence h_{t-1} -> h_t
 * (public/GRU_Spatial.py:170-178) EXPANDS perturbations: a float32 forward pass, whatever its summation order, leaves a 50-position
 * sequence 1e-5 off the float64 result, and the whole update with it; the backward pass is linear in its carry and is not affected.
 * on = 1: the input product ui . x_t + bi and the recurrent products are computed in ~40-bit fixed point on the INT8 matrix cores
 * (five signed base-256 digit planes per operand, exact int32 accumulation, digit pairs combined in float64: te_xfwd.hip), the gates
 * and the state in float64; everything behind the forward pass (head, BPTT, gradients, write-back) stays float32 and reads the
 * float32 roundings of z, r, c, h.  on = 0: the float32 forward kernels of rounds 1 - 3 (split products / per-sequence / forward table).
 * Dim 256 (config X of BASELINE.json; round 5): the input product keeps the digit-pair classes 0 .. 6 (22 int8 MFMAs per 32 k: ~2^-55) and the
 * recurrence runs in float64 on the matrix cores (v_mfma_f64_16x16x4_f64, float32 weight fragments streamed from L2: te_rec_fwdd) - with the
 * reference's init at that dim the chain amplifies a perturbation ~10^6-fold over 50 positions and nothing less holds 1e-5.
 * A NaN / inf weight or input row makes every hidden state, loss and updated tensor of the launch NaN (the float64 reference propagates it
 * to everything that depends on it; the int8 digits of a state cannot carry it, so the launch is flagged while its operands are prepared).
 * per_sequence_max (>= 0; < 0 keeps the current value, default 1100; dims 64 / 128): launches of at most this many sequences run the recurrence
 * per sequence in float64 on the vector ALUs (te_rec_fwd1x: persistent workgroups, one per CU, walk the launch's sequences with the weights in
 * registers; the reference's schedule - one user per step, prog_bpr_gru_spatial.py:249-250 - takes this form), larger ones in 16-sequence tiles
 * on the int8 matrix cores (te_rec_fwdx: 3.6 us per step and tile).  Environment overrides at context creation: POI_TE_XFWD=0|1, POI_TE_XREC1=<per_sequence_max>. */
int poi_ctx_set_exact_forward(poi_ctx* ctx, int on, int per_sequence_max);
/* Named tuning switches of the tile engine - every setting computes the same update to the stated tolerances; they exist for A/B
 * measurements and for the tests that hold the alternative kernels to the oracle.  POI_EINVAL for an unknown name or a value out of range.
 *   "forward_table_compact" 0|1 (default 1): the exact forward pass forms its float64 input table over the POIs that are step inputs
 *       of the launch only (ranked on the device) instead of over every row of the POI table - bitwise the same update;
 *   "forward_table_compact_min" n (default 1536): ... for launches of at least n sequences;
 *   "xfwd_ids_lds" 0|1 (default 1): the table-form recurrences of the exact forward pass (forward table / compact table: te_rec_fwdxi, te_rec_fwddi,
 *       te_rec_fwd1xi) stage the table-row ids of their sequences' steps in LDS once per tile / sequence instead of loading them inside the step
 *       loop, where the wait for them also drained the step's stores - bitwise the same update; 0, or an id table that does not fit the
 *       kernel's LDS (16-sequence tiles at dim 128: more than 133 steps), takes the in-loop loads;
 *   "stream_hints" 0|1 (default 1), "stream_hints_min" n (default 2560): in training launches of at least n sequences (dim 128; 2 n at dim 64:
 *       the bound is one of bytes) the 16-sequence tiles of the exact forward recurrence store the per-step rows G, H and RH - written once, read by later kernels only - with the
 *       non-temporal policy, so that they do not displace the forward table's rows from the caches - bitwise the same update; smaller launches
 *       keep plain stores (their rows stay on-die for the backward recurrence);
 *   "head_split" 0|1 (default 1): the training head (public/GRU_Spatial.py:180-200, <= 256 bins) on bf16 split products (te_head3)
 *       instead of float32-input matrix instructions;
 *   "early_bins" 0|1 (default 1): the distance-bin rows' write-back chain starts next to the d x product instead of at the tail;
 *   "hot_bins" 0|1 (default 1; ABI 5): the per-POI pass over DA also sums the rows of the (<= 4) most frequent step-input distance bins of the
 *       launch - on check-in data a few bins hold most steps - so the per-bin pass reads only the rows of the others; reproducible,
 *       another fixed summation order than 0;
 *   "hybrid" 0|1 (default 1; ABI 6), "hybrid_min" / "hybrid_max" n (defaults 1150 / 2300): training launches of hybrid_min .. hybrid_max sequences at
 *       dim 128 run their two recurrences (public/GRU_Spatial.py:170-178 and its BPTT) on BOTH kernel families at once - the longest sequences of the
 *       launch one per workgroup (float64 / float32 FMAs: 2.6 / 1.35 us per step) on a second stream while the shorter rest runs in 16-sequence matrix-core
 *       tiles (4.5 / 2.9 us per step) on the other CUs; the split is chosen on the device from the launch's own lengths.  A 1563-sequence launch is 98
 *       tiles - 158 CUs idle behind the longest tile's 49-step chain: 678 -> 632 us.  Every sequence still goes through one of the two kernel
 *       families that hold it to the oracle on their own; a sequence's values depend on which one (inside the bars), identical launches are bitwise
 *       identical.  "hybrid_force" n (tests): n leading sequences per workgroup whatever the cost model says;
 *   "session_tile_min" n (default 512): poi_session_advance calls of at least n events take the 16-event tile kernel.
 *   "cell_grid" n (default 0 = no cap): poi_cell_step / poi_cell_predict run their recurrent kernel on at most n workgroups (the persistent
 *       grid is min(sequences, 512) otherwise) - bitwise the same result for every n.
 *   "vbpr_grid" n (default 0 = no cap): every kernel of poi_vbpr_step / poi_vbpr_items runs on at most n workgroups - bitwise the same
 *       result for every n (tests).
 *   "near_split_max" n (default 256): poi_score_topk_near calls of at most n rows cut every row's band into slices, a workgroup each, and
 *       merge the slices' lists (0: never); larger calls run one workgroup per row;
 *   "near_grid" n (default 0 = by the row count and the CUs; at most 64): slices per row on that split path - bitwise the same result for
 *       every n and on either path.
 *   "rank_grid" n (default 0 = by the row count and the CUs): poi_score_rank splits the item range of a 32-row tile over at most n
 *       wavefronts (never fewer than ceil(item tiles / 65535)) - identical ranks for every n.
 *   "group_split_max" n (default 256): poi_group_topk calls of at most n groups cut the item range into slices, a workgroup each, and merge
 *       the slices' lists (0: never); larger calls run one workgroup per 8 groups;
 *   "group_grid" n (default 0 = by the group count and the CUs; at most 64): slices on that split path - bitwise the same result for
 *       every n and on either path.
 *   "route_split_max" n (default 8192 = 32 rows for each of 256 CUs): poi_route_expand calls of at most n rows cut the item range of every
 *       32-row tile over several workgroups and finish the rows in a second kernel (0: never); larger calls run one workgroup per tile;
 *   "route_grid" n (default 0 = by the row count and the CUs; at most 64): workgroups per 32-row tile on that split path - bitwise the
 *       same result for every n and on either path.
 *   "diverse_split_max" n (default 256): poi_diverse_pool / poi_diverse_topk calls of at most n rows cut the item range of every 32-row tile
 *       into slices, a workgroup each, and merge the slices' lists (0: never); larger calls run one workgroup per tile;
 *   "diverse_grid" n (default 0 = by the row count and the CUs; at most 64): slices on that split path - bitwise the same result for
 *       every n and on either path.
 *   "select_split_max" n (default 256): poi_topk_select / poi_score_candidates calls of at most n rows cut each row's id range into
 *       slices, a workgroup each (0: never); larger calls run one workgroup per row;
 *   "select_grid" n (default 0 = by the row count and the CUs; at most 64): slices on that split path - bitwise the same result for
 *       every n and on either path;
 *   "select_chunk_mb" n (default 1024, at least 1): poi_score_candidates keeps at most n MiB of score rows at a time (a whole number
 *       of 32-row tiles, at least one) - bitwise the same result for every n;
 *   "audience_split_max" n (default 256): poi_score_audience / poi_audience_rows calls of at most n query POIs cut the candidate rows
 *       into slices, one workgroup per (32-query block, slice), and merge the slices' lists (0: never); larger calls run one workgroup
 *       per query block;
 *   "audience_grid" n (default 0 = by the query-block count and the CUs; at most 64): slices in that split regime - bitwise the same
 *       result for every n and in either regime;
 *   "similar_split_max" n (default 16384) / "similar_grid" n (default 0; at most 64): the same two for poi_similar_topk /
 *       poi_similar_rows - queries in the query POIs' place, the table's own rows in the candidate rows'.  The default is where two
 *       workgroups per CU leave one slice anyway: one workgroup per query block walks the whole table alone, which costs the
 *       same few milliseconds for 257 queries as for 8192;
 *   "similar_rows_max" n (default 1024, at most 4096): poi_similar_topk calls of at most n queries write their score rows
 *       (poi_similar_rows' walk) and select from them (poi_topk_select's kernels) instead of keeping fused lists - for few queries the
 *       faster route; 0: never.  Bitwise the same result for every n;
 *   "capped_split_max" n (default 256) / "capped_grid" n (default 0 = by the row count and the CUs; at most 64): the split regime
 *       of poi_score_topk_capped and its slices, as "filter_split_max" / "filter_grid" are the walk path's of
 *       poi_score_topk_filtered - bitwise the same result for every n and in either regime;
 *   "capped_hist_kb" n (default 262144 = 256 MiB): poi_labels_build keeps at most n KiB of per-predicate label histograms
 *       ((n_label + 1) ints per predicate) in the context's workspace at a time - whole predicates, at least one; more predicates go
 *       through it in chunks.  The same tables for every n;
 *   "labels_split_max" n (default 256) / "labels_grid" n (default 0 = by the row count and the CUs; at most 64): the split regime of
 *       poi_score_labels / poi_score_topk_labels and its slices, as "capped_split_max" / "capped_grid" - bitwise the same result;
 *   "labels_lds_kb" n (default 40, at most 120; 0: never): the label accumulators of a workgroup (32 rows x (n_label + 1) buckets x 20
 *       bytes; poi_labels_scores: one row) live in LDS and are flushed once while they fit n KiB, otherwise every candidate goes to the
 *       context's global accumulator with integer atomics - bitwise the same result on either side;
 *   "labels_ws_kb" n (default 262144 = 256 MiB): the global accumulator holds at most n KiB (whole 32-row tiles, at least one); more
 *       rows go through it in chunks.  Bitwise the same result for every n;
 *   "explain_start" 0 | 1 (default 1): poi_explain_loo starts a variant from the base walk's checkpoint before its first removed
 *       position (1) or at position 0 from h = 0 (0).  Bitwise the same result on either side. */
int poi_ctx_set_option(poi_ctx* ctx, const char* name, int value);
/* Small launches: launches of at most max_sequences sequences (default 1800; 0 disables; dim 64 / 128) run the recurrence of every
 * sequence per workgroup on the vector ALUs (te_rec_fwd1 / bwd1, weights resident in registers; persistent since round 5: one workgroup per
 * CU slot walks the launch's sequences) instead of 16-sequence MFMA
 * tiles - a tile step costs the same whether it holds 16 sequences or one, so the reference schedule (one user per step,
 * prog_bpr_gru_spatial.py:249-250) and launches that do not fill the chip are bound by it.  Same formulas, float32 FMA chains; the
 * summation order differs from the tile kernels.  Environment override at context creation: POI_TE_REC1=<max_sequences>. */
int poi_ctx_set_small_launch(poi_ctx* ctx, int max_sequences);
/* Regrouped backward pass (per-bin tables, per-POI regrouping, forward table: DESIGN.md section 5) only for launches of at least
 * min_sequences sequences (default 1280; dim >= 128, Distance2Pre): the regroupings trade matrix work for sorting / segmented-sum
 * dispatches, which pays from ~1500 sequences per launch; smaller launches take the two-table path (the step input gathered from lt | di
 * inside the GEMMs) - 16 users: 342 -> 277 us per launch, 256 users: 393 -> 323 us.  Same formulas, same batch rule.  0 = always regroup.
 * Environment override at context creation: POI_TE_BINTAB_MIN=<min_sequences>. */
int poi_ctx_set_regroup_min(poi_ctx* ctx, int min_sequences);
/* One-sequence path (default on): a poi_spatial_step / poi_gru_step launch of ONE sequence - the reference schedule, prog_bpr_gru_spatial.py:249-250 -
 * at dim 64 / 128 (stored dims below are padded), float32 tables, sequences of at most 161 positions (the reference mentions len_max 157 for Foursquare), runs the whole step in five
 * kernels instead of the batched pipeline's ~40 dispatches (input products on the vector ALUs, per-sequence recurrences, the head,
 * and ONE kernel for every gradient product with the SGD step in its epilogue and the sparse write-back, one workgroup per table
 * touch).  Same formulas and write-back rule (public/GRU_Spatial.py:127-229); on = 0 sends such launches through the batched
 * pipeline.  Needs poi_ctx_set_small_launch >= 1.  Environment override at context creation: POI_TE_ONE=0|1. */
int poi_ctx_set_one_sequence_path(poi_ctx* ctx, int on);

/* Seeded top-K (optional, exact): seed_idx (n x k_seed int32, device) holds, for every user of the NEXT fused top-K call
 * (poi_score_topk / _ulptai / _geo with the same n and user order), k_seed >= k distinct item ids - typically the user's top-K of the
 * previous evaluation (public/Valuate.py runs after every epoch; the lists barely move).  The seed items' scores under the current
 * model, minus a float32 rounding bound, are a lower bound of the user's K-th best score; the scoring kernels start from it instead
 * of -inf and insert little more than the final top-K.  The result is the exact top-K whatever the seed holds (rows with an id
 * outside [0, n_item) or a repeated id are simply not seeded).  Consumed by the next call; NULL clears. */
int poi_ctx_set_topk_seed(poi_ctx* ctx, const int32_t* seed_idx, int32_t k_seed);
/* Two-stage fused top-K (default on; POI_TOPK_FILTER=0 / on = 0: the one-stage float32 kernel only).  A poi_score_topk /
 * poi_score_topk_ulptai / poi_score_topk_geo call (no dense prob matrix, <= 1023 bins, >= 128 users) runs a FILTER pass on half-rounded users / items
 * (v_mfma_f32_32x32x16_f16, 16x the float32 matrix rate) with a rigorous bound on |approximate - float32 score| per pair, keeps the pairs
 * that could beat the user's seeded threshold (~K + a few per user), and rescores exactly those with the one-stage kernel's own float32
 * MFMA sequence and distance term: the same ids AND scores, bit for bit.  The path seeds itself: unseeded calls first run the one-stage
 * kernel on the first 1/16 of the item tiles (any subset's K-th best exact score is a valid threshold); seeded calls do the same on 1/64
 * when the table has >= 2^20 items, so a useless seed costs nothing but survivors.  User tiles whose survivor lists still overflow
 * (4096 slots per user) are handed to the one-stage kernel.  poi_score_topk_geo: dims 64 / 128 / 256, bins computed on the fly; with
 * >= 2^20 items and <= 131072 users (config X's evaluation) its filter pass is ITEM-stationary - a workgroup keeps four item tiles in
 * registers and walks the user tiles, whose half fragments are L2-resident, instead of every user tile walking the item table.
 * on = 2 / 3: two-stage with the item-stationary GEO filter forced / forbidden (tests, A/B runs; POI_SF_ITEMS=1|0). */
int poi_ctx_set_topk_filter(poi_ctx* ctx, int on);
/* Host-side statistics of the LAST two-stage call (synchronises): users scored, pairs the filter kept (all users), 32-user tiles, and the
 * tiles whose survivor lists overflowed and were handed to the one-stage kernel.  users == 0: no two-stage call so far. */
int poi_ctx_topk_filter_stats(poi_ctx* ctx, int64_t* users, int64_t* survivors, int64_t* tiles, int64_t* tiles_flagged);

/* Batch rule cap (>= 1, see "Batch semantics" above); applies to poi_spatial_step / poi_gru_step / poi_bpr_step
 * (snapshot mode) / poi_fpmc_step / poi_prme_step launches with more than one sequence.  n_seq == 1 is the reference step for every cap.
 * cap == 0 selects the MINI-BATCH rule of the reference's `Gru` class (public/GRU.py:395-498, cost :452-459): the launch is one
 * mini-batch - loss gradients averaged over its n sequences, L2 terms of every gathered row (all len_max positions of every
 * sequence, duplicates counted) summed: row -= alpha (G / n + lambda mult row); dense tensors: theta -= alpha (G / n + lambda theta).
 * poi_gru_step / poi_spatial_step only (POI_ENOTSUP elsewhere). */
int poi_ctx_set_batch_cap(poi_ctx* ctx, float cap);

/* ---- a5: BPR-MF step - OboBpr.bpr_train(uidx, [p, q]), public/BPR.py:201-241 ----------------
 * n independent (user, positive, negative) triples.  ux (n_user, D), lt (n_item+1, D).
 * loss_out[n] = -log sigmoid(u).  mode: POI_BPR_SNAPSHOT = batch semantics above - every triple at the launch-entry
 * values; the 3 n table touches are sorted by row and summed in a fixed order (no float atomics: identical launches give
 * bitwise identical tables; ABI 5); lt may be a registered IEEE-half table (float32 arithmetic, poi_ctx_set_f16_rounding
 * applies), ux stays float32; dim a multiple of 4 up to 1024.
 * POI_BPR_HOGWILD = in-place racy update (one pass over the three rows; identical to the
 * reference whenever no row is shared inside the launch, e.g. n == 1; float32 tables only).
 * A triple with an id outside its table is rejected (ABI 6): NaN loss, counted once per triple, and - snapshot mode - the launch
 * equals the launch without it bit for bit: no gradient, no L2 decay, no multiplicity on any row. */
enum { POI_BPR_SNAPSHOT = 0, POI_BPR_HOGWILD = 1 };
int poi_bpr_step(poi_ctx* ctx, float* ux, float* lt, int32_t n_user, int32_t n_item, int32_t dim,
                 const int32_t* uidx, const int32_t* p, const int32_t* q, int32_t n,
                 float alpha, float lambda, float* loss_out, int mode, void* stream);

/* ---- a2: Distance2Pre step - OboSpatialGru.seq_train(uidx), public/GRU_Spatial.py:127-229 ---
 * uidx[n_seq] = user ids (rows of the CSR tables) trained in this launch.
 * out[5*k .. 5*k+4] = [los, sur, upq, ls0, ls1] of sequence k (the 4-tuple the reference returns,
 * public/GRU_Spatial.py:222, with ls flattened). */
int poi_spatial_step(poi_ctx* ctx, const poi_gru_params* prm, const poi_seq_tables* tab,
                     const int32_t* uidx, int32_t n_seq, float alpha, float lambda,
                     float* out, void* stream);

/* ---- a4: plain GRU + BPR step - OboGru.seq_train(uidx), public/GRU.py:313-389 ---------------
 * out[k] = -sum_t log sigmoid(u_t) (public/GRU.py:380). */
int poi_gru_step(poi_ctx* ctx, const poi_gru_params* prm, const poi_seq_tables* tab,
                 const int32_t* uidx, int32_t n_seq, float alpha, float lambda,
                 float* out, void* stream);

/* ---- f4: CA-RNN (flag 3) - OboCARNN, public/CA_RNN.py:46-227 ----------------------------------
 * lt (n_item+1, D), wd (n_dist+1, H, D) interval-specific transition matrices, M (H, D); H == D (the driver passes
 * n_in == n_hidden, prog_bpr_gru_spatial.py:148-149).  h0 is the zero vector (never trained).
 * poi_carnn_step: seq_train(uidx), :105-170 - out[k] = los = -sum_t log sigmoid(yp_t - yq_t); sparse write-back of the
 *   unique rows of p U q (lt) and of the unique interval MATRICES of dp U dq (wd), dense update of M; batch rule as above.
 *   dim 64 / 128: the recurrence kernel records the step vectors and every gradient (interval matrices, M, POI rows) is a sorted,
 *   fixed-order sum on the matrix cores - no float atomics, bitwise reproducible; other dims: one kernel per sequence with float
 *   atomics on the gradient tables (POI_CARNN_FAST=0 forces it).
 * poi_carnn_predict: seq_predict(start_end), :172-217, literally (the predict graph adds-then-sums, :191:
 *   h_t = sigmoid(M p_t + rowsum(wd[d_t]) + sum(h_{t-1}))); prm->lt / prm->wd must point at the snapshots.
 * poi_carnn_score_all: compute_sub_all_scores(start_end), :91-101, literally:
 *   score[u][j] = -( sum(wd[bin(u, j)]) + H * sum(users[u]) + sum(M . items[j]) ),  bin(u, j) = the reference's
 *   usrs_last_poi_to_all_intervals entry, computed on the fly from coords / cphi / thr (as poi_dist_prob) - the U x N
 *   matrix is never materialised.  scores_out (n, n_item). */
typedef struct poi_carnn_params { float* lt; float* wd; float* M; int32_t n_item; int32_t n_dist; int32_t dim; } poi_carnn_params;
int poi_carnn_step(poi_ctx* ctx, const poi_carnn_params* prm, const poi_seq_tables* tab, const int32_t* uidx, int32_t n_seq,
                   float alpha, float lambda, float* out, void* stream);
int poi_carnn_predict(poi_ctx* ctx, const poi_carnn_params* prm, const poi_seq_tables* tab, const int32_t* uidx, int32_t n,
                      float* hts, void* stream);
int poi_carnn_score_all(poi_ctx* ctx, const float* users, const float* items, const float* M, const float* dists, const double* coords,
                        const double* cphi, const double* thr, const int32_t* last_poi, int32_t n, int32_t n_item, int32_t n_dist,
                        int32_t dim, double dd, float* scores_out, void* stream);

/* ---- a6: predict - seq_predict(start_end), public/GRU_Spatial.py:231-288, public/GRU.py:154-205
 * prm->lt / prm->di must point at the SNAPSHOTS trained_items / trained_dists.
 * hts (n, D) = hidden state after the user's whole train sequence; sts (n, n_dist+1) =
 * softmax(vs.h + bs) (spatial only; pass NULL for OboGru).
 * out_row (n, device) or NULL: the result of uidx[k] is written to output row out_row[k] instead of k - the caller
 * can hand the users over sorted by descending length (a 16-sequence recurrent tile runs for its longest member) and
 * still receive the rows in its own order, with no gather / scatter pass of its own. */
int poi_gru_predict(poi_ctx* ctx, const poi_gru_params* prm, const poi_seq_tables* tab,
                    const int32_t* uidx, const int32_t* out_row, int32_t n, float* hts, float* sts, void* stream);

/* ---- a8: all-POI scoring - compute_sub_all_scores(start_end) --------------------------------
 * public/GRU.py:93-96, public/BPR.py:76-79; spatial variant adds wd*prob, public/GRU_Spatial.py:117-125.
 * users (n, D) rows already selected (trained_users[start_end]); items (n_item+1, D) = trained_items
 * (padding row dropped); prob (n, n_item) or NULL; wd read from device (NULL with prob NULL).
 * scores_out (n, n_item) row-major. */
int poi_score_all(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item,
                  int32_t dim, const float* wd, const float* prob, float* scores_out, void* stream);

/* ---- a8+a9 fused: scoring + top-K - public/Valuate.py:91-100,132-146 -----------------------
 * Same score definition as poi_score_all; the (n, n_item) matrix is never materialised.
 * idx_out (n, k) int32 sorted by descending score, ties by ascending index; score_out (n, k) or NULL.
 * An item whose score is -inf or NaN is never selected (every comparison is `score > threshold`, from -inf): a row with fewer than k
 * selectable items ends in -1 ids and -inf scores, as poi_score_topk_near states it.  The same holds for poi_score_topk_ulptai and
 * poi_score_topk_geo, one- and two-stage.  A K-th best of exactly +0.0 is a score like any other (ties at zero are kept); how a -0.0
 * score ranks against +0.0 scores is NOT specified (the candidate lists order -0.0 below +0.0, the merge treats them as equal).
 * tests: tests/test_gpu_topk_adversarial.py (planted ties, plateaus across item ranges, short rows, NaN). */
int poi_score_topk(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item,
                   int32_t dim, const float* wd, const float* prob, int32_t k,
                   int32_t* idx_out, float* score_out, void* stream);

/* ---- a9 alone: top-K of a given score matrix, k <= 64 (checks the selection independently of the GEMM; also the path for
 * cut-offs beyond the fused kernels' k <= 32, e.g. at_nums = [5, 10, 15, 20, 30, 50] of public/Valuate.py:126).
 * Order and short rows as poi_score_topk: descending score, ties by ascending index; -inf and NaN entries are never selected, and a
 * row with fewer than k selectable entries ends in -1 ids and -inf scores. */
int poi_topk(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, int32_t k,
             int32_t* idx_out, float* score_out, void* stream);

/* ---- a10: AUC preference - compute_sub_auc_preference(start_end), public/GRU.py:98-110 ------
 * users (n, D); tes_p/tes_q/tes_mask (n, len_tes) int32; out (n, len_tes) uint8 = (u.(xp-xq))*mask > 0 */
int poi_auc_preference(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t dim,
                       const int32_t* tes_p, const int32_t* tes_q, const int32_t* tes_mask,
                       int32_t len_tes, uint8_t* out, void* stream);

/* ---- model.l2.eval(): sum of squares of a flat buffer (public/GRU_Spatial.py:83-88) ----------
 * out[0] += sum x^2 (out is a device float64 accumulator the caller zeroes). */
int poi_sumsq(poi_ctx* ctx, const float* x, int64_t n, double* out, void* stream);

/* usrs_last_poi_to_all_intervals ("ulptai"): the reference computes the distance bin of every (user's last train
 * POI, POI) pair ONCE per data set (prog_bpr_gru_spatial.py:90, fun_compute_distance, public/Load_Data_by_length.py:
 * 183-216) and every evaluation only gathers prob[u][j] = sus[u][ulptai[u][j]] (zero where the bin is >= n_dist;
 * fun_acquire_prob, :218-235, prog_bpr_gru_spatial.py:288).  poi_ulptai_build fills the resident bin matrix on the
 * device with the exact host thresholds of poi_dist_prob (cphi, thr); bin_bytes = 1 (n_dist <= 255) or 2.  Layout:
 * 32-user x 32-POI tiles of 1024 bins in the order the scoring kernel consumes them,
 *   out[((ut * ntile + it) * 64 + lane) * 16 + r],  user = 32 ut + (r&3) + 8 (r>>2) + 4 (lane>>5),  POI = 32 it + (lane&31),
 * ntile = ceil(n_item / 32); size ceil(n_user/32) * ntile * 1024 * bin_bytes bytes; out-of-range pairs hold n_dist. */
int poi_ulptai_build(poi_ctx* ctx, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                     int32_t n_user, int32_t n_item, int32_t n_dist, double dd, void* out, int32_t bin_bytes, void* stream);

/* poi_score_topk with the distance term taken from the resident bin matrix instead of a dense float `prob`:
 *   score[u][j] = users[u] . items[j] + wd * (bin < n_dist ? sts[u][bin] : 0),  bin = ulptai[u][j]
 * (compute_sub_all_scores, public/GRU_Spatial.py:117-125, after fun_acquire_prob + update_prob).  `ulptai` points at
 * the tile row of the batch's first user (the batch must start at a multiple of 32 users).  sts is the batch's
 * (n, n_dist + 1) bin-probability table with the mask of fun_acquire_prob folded in: column n_dist ("too far") must
 * hold 0, and the buffer must be readable for ceil(n / 32) * 32 rows (whole user tiles; the extra rows' values are
 * irrelevant). */
int poi_score_topk_ulptai(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                          const float* wd, const float* sts, const void* ulptai, int32_t bin_bytes, int32_t n_dist,
                          int32_t k, int32_t* idx_out, float* score_out, void* stream);

/* The same score with the bins computed ON THE FLY from the coordinates inside the scoring kernel (float64 Haversine `c` in the
 * reference's operation order + the exact host thresholds of poi_dist_prob): neither the reference's U x N bin matrix nor a dense
 * prob matrix is ever materialised - the form for tables where U x N bytes cannot exist (config X: 1 M users x 10 M POIs), any
 * dim <= 256, any batch start.  last_poi (n) = the batch users' last train POI; sts as for poi_score_topk_ulptai (column n_dist
 * zero, readable for whole 32-user tiles). */
int poi_score_topk_geo(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim, const float* wd,
                       const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                       int32_t n_dist, double dd, int32_t k, int32_t* idx_out, float* score_out, void* stream);

/* ---- last-train-POI -> all-POI distance-bin probability rows (8f rank 2) ---------------------
 * public/Load_Data_by_length.py:183-235 (fun_compute_distance + fun_acquire_prob) for a user batch:
 * prob_out[k][j] = sts[k][bin] * (bin < n_dist), bin = cal_dis(coord[last_poi[k]], coord[j]).
 * coords (n_item, 2) float64 lat,lon; sts (n, n_dist+1) float32; dd in metres.
 * Fast exact path: cphi (n_item) float64 = cos(lat*pi/180) and thr (n_dist) float64 = the smallest
 * Haversine `c` at which each bin starts, both precomputed on the host with the reference's libm
 * (data.py cos_lat / bin_thresholds); then no asin/sqrt runs on the device and the bins equal
 * cal_dis for every c.  With cphi == thr == NULL the kernel evaluates cal_dis literally. */
int poi_dist_prob(poi_ctx* ctx, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                  const float* sts, int32_t n, int32_t n_item, int32_t n_dist, double dd, float* prob_out, void* stream);

/* ---- rank metrics on the device (8f rank 3) - public/Valuate.py:23-88,149-172 --------------------
 * ranks (n, k) int32 (descending score); tes_p / tes_mask (n, len_tes); at_nums (n_at <= 8, ascending,
 * <= k, device int32).  acc (n_at, 3) float64, caller-zeroed, receives SUMS over the n users of
 * [hits, average precision, NDCG] at each cut-off (recall = hits / sum(mask), precision = hits/(k n),
 * MAP / NDCG = sums / n_user, as Valuate.py:155-172). */
int poi_rank_metrics(poi_ctx* ctx, const int32_t* ranks, int32_t n, int32_t k, const int32_t* tes_p, const int32_t* tes_mask,
                     int32_t len_tes, const int32_t* at_nums, int32_t n_at, double* acc, void* stream);

/* ---- per-epoch negative refresh on the device (8f rank 1) --------------------------------------
 * poi_sample_negatives: fun_random_neg_masks_tra / _tes, public/Load_Data_by_length.py:127-162, called
 * every epoch by prog_bpr_gru_spatial.py:221-222.  q_out (flat, CSR) gets one uniform draw over
 * [0, n_item) per train position, redrawn while it equals one of the user's train items;
 * tes_q_out (n_user, len_tes) or NULL likewise, also avoiding the user's test items (padded test
 * positions keep n_item).  Counter-based RNG: same (seed, data) -> same output.
 * poi_neg_dist_bins: fun_compute_dist_neg, :165-180 - dq[t] = cal_dis(neg_t, pos_{t-1}), dq[0] = n_dist,
 * with the exact host thresholds of poi_dist_prob (cphi, thr). */
int poi_sample_negatives(poi_ctx* ctx, const int32_t* off, const int32_t* p, int32_t n_user, int32_t n_item, const int32_t* tes_p,
                         const int32_t* tes_mask, int32_t len_tes, uint64_t seed, int32_t* q_out, int32_t* tes_q_out, void* stream);
int poi_neg_dist_bins(poi_ctx* ctx, const int32_t* off, const int32_t* p, const int32_t* q, int32_t n_user, const double* coords,
                      const double* cphi, const double* thr, int32_t n_dist, double dd, int32_t* dq_out, void* stream);

/* ---- FPMC-LR (ABI 7) - prog_fpmc_lr.py, public/FPMC_LR.py, public/Load_Data_fpmc_lr.py -----------------------------------
 * Neighbour sets (fun_acquire_neighbors_for_each_poi, Load_Data_fpmc_lr.py:114-143): neighbours(i) = {k != i : cal_dis(i, k) <= UD},
 * CSR over POI ids: row i = nbr[off[i] .. off[i+1]), int64 offsets (totals may pass 2^31).  coords (n_item, 2) float64 lat, lon;
 * cphi (n_item) = cos(lat * pi / 180) with the reference's libm (data.cos_lat); lat_order (n_item) = the POI ids in ascending latitude
 * (a stable argsort); c_ud = data.ud_threshold(UD): the smallest Haversine c at which 12742 asin(sqrt(c)) > UD, so that
 * c < c_ud <=> dist <= UD for every c and no asin / sqrt runs on the device.  c is evaluated in float64 in cal_dis's operation order
 * (as poi_dist_prob); a query scans only the latitude band that can hold neighbours.
 * poi_fpmc_neighbor_counts writes off_out (n_item + 1) - off_out[n_item] is the total; the caller reads it, allocates nbr (or refuses)
 * and calls poi_fpmc_neighbor_fill with the same arguments.  Row order: ascending position in lat_order; the output is deterministic. */
int poi_fpmc_neighbor_counts(poi_ctx* ctx, const double* coords, const double* cphi, const int32_t* lat_order, int32_t n_item, double c_ud,
                             int64_t* off_out, void* stream);
int poi_fpmc_neighbor_fill(poi_ctx* ctx, const double* coords, const double* cphi, const int32_t* lat_order, int32_t n_item, double c_ud,
                           const int64_t* off, int32_t* nbr_out, void* stream);
/* Training negatives (prog_fpmc_lr.py:188-190, random.sample(negs[i+1], 1), redrawn every epoch): neg_out[t] = one uniform draw from
 * neighbours(pos[t]), nbr[off[i] + floor(r cnt(i))], r from the counter-based RNG of poi_sample_negatives keyed on (seed, t): the same seed
 * gives the same output.  A position outside [0, n_item) or a POI without neighbours gets -1 (which poi_fpmc_step rejects). */
int poi_fpmc_sample_negatives(poi_ctx* ctx, const int64_t* nbr_off, const int32_t* nbr, int32_t n_item, const int32_t* pos, int64_t n,
                              uint64_t seed, int32_t* neg_out, void* stream);
/* Tables (FPMC_LR.py:52-59): ui (n_user, D); iu, ia, ai (n_item + 1, D) with a padding row.  Float32 only; D a multiple of 4, D <= 128 (the
 * evaluation scores [ui | ai[last]] . [iu | ia] at width 2 D <= 256 with poi_score_all / poi_score_topk / poi_auc_preference). */
typedef struct poi_fpmc_params {
  float* ui; float* iu; float* ia; float* ai;
  int32_t n_user; int32_t n_item; int32_t dim;
} poi_fpmc_params;
/* n transitions (u, a = POI at t-1, i = POI at t, j = negative), FPMC_LR.py:113-151:
 *   x = ui[u].(iu[i] - iu[j]) + ai[a].(ia[i] - ia[j]),  s = sigmoid(-x),  loss_out[t] = log sigmoid(x)  (the driver sums it as is)
 *   ui[u] += alpha (s (iu[i] - iu[j]) - lambda ui[u])    ai[a] += alpha (s (ia[i] - ia[j]) - lambda ai[a])
 *   iu[i] += alpha (s ui[u] - lambda iu[i])               iu[j] += alpha (-s ui[u] - lambda iu[j])
 *   ia[i] += alpha (s ai[a] - lambda ia[i])               ia[j] += alpha (-s ai[a] - lambda ia[j])
 * every right-hand side at the launch-entry values; batch semantics above (poi_ctx_set_batch_cap), a row's touches within one table
 * counted together (iu[r] as a positive and as a negative: k = 2); n == 1 is the reference step.  The 6 n touches are sorted by
 * (table, row) and summed in a fixed order with no float atomics: identical launches give bitwise identical tables.  A transition with
 * u outside [0, n_user), a / i / j outside [0, n_item], or i == j moves nothing (no gradient, no decay, no multiplicity), its loss is NaN
 * and it is counted once (poi_ctx_take_bad_ids).  Timing names: "fpmc_nbr_count", "fpmc_nbr_fill", "fpmc_sample", "fpmc_fwd", "fpmc_sort",
 * "fpmc_rows", "fpmc_commit". */
int poi_fpmc_step(poi_ctx* ctx, const poi_fpmc_params* prm, const int32_t* u, const int32_t* a, const int32_t* i, const int32_t* j, int32_t n,
                  float alpha, float lambda, float* loss_out, void* stream);

/* ---- PRME (ABI 8) - prog_prme.py, public/PRME.py (public/PRPRM.py: the same maths), public/Load_Data_prme.py -------------------
 * Tables (PRME.py:75-82): du (n_user, D); dp, ds (n_item + 1, D) with a padding row.  Float32 only; D a multiple of 4, D <= 128. */
typedef struct poi_prme_params {
  float* du; float* dp; float* ds;
  int32_t n_user; int32_t n_item; int32_t dim;
} poi_prme_params;
/* n transitions (u, p = POI at i, q = negative, prev = POI at i-1, d = dist[i] float64 km, gap[i] minutes), replacing OboPrme.train
 * (PRME.py:173-219, driver prog_prme.py:191-197):
 *   far = gap > threshold,  w = (1 + d)^0.25,  a = far ? 1 : w cw,  b = far ? 0 : w (1 - cw)
 *   x = a (|du-dp_q|^2 - |du-dp_p|^2) + b (|ds_q-ds_prev|^2 - |ds_p-ds_prev|^2),  loss_out[t] = log sigmoid(x),  g = sigmoid(-x)
 *   du += alpha (2a g (dp_p - dp_q) - lambda du)          dp_p += alpha (2a g (du - dp_p) - lambda dp_p)
 *   dp_q += alpha (-2a g (du - dp_q) - lambda dp_q)       dp_prev += alpha (-lambda dp_prev)
 *   ds_p += alpha (-2b g (ds_p - ds_prev) - lambda ds_p)  ds_q += alpha (2b g (ds_q - ds_prev) - lambda ds_q)
 *   ds_prev += alpha (2b g (ds_p - ds_q) - lambda ds_prev)
 * every right-hand side at the launch-entry values.  A repeated row within one transition keeps the LAST occurrence in the order
 * (p, q, prev) - Theano's set_subtensor: with p == prev, dp[p] moves by decay only and ds[p] takes the prev occurrence's update - and
 * then counts as one touch.  Batch semantics above (poi_ctx_set_batch_cap); n == 1 is the reference step.  The 7 n touches are sorted by
 * (table, row) and summed in a fixed order with no float atomics: identical launches give bitwise identical tables.  A transition with
 * u outside [0, n_user), p / q / prev outside [0, n_item], p == q, or d not finite or < 0 moves nothing, its loss is NaN and it is
 * counted once (poi_ctx_take_bad_ids).  Timing names: "prme_fwd", "prme_sort", "prme_rows", "prme_commit". */
int poi_prme_step(poi_ctx* ctx, const poi_prme_params* prm, const int32_t* u, const int32_t* p, const int32_t* q, const int32_t* prev,
                  const double* d, const int32_t* gap, int32_t n, float alpha, float lambda, int32_t threshold, float cw, float* loss_out,
                  void* stream);
/* Geo-weighted all-POI scores, replacing PrmeBasic.compute_sub_all_scores (PRME.py:117-139): prm holds the trained snapshots
 * (du, dp with at least n_item rows, ds with n_item + 1); coords (n_item + 1, 2) float64 lat, lon, row n_item the pad POI (0, 0).
 * Output row r is (users[r], query POI qpoi[r] in [0, n_item]); for a candidate j < n_item
 *   out[r][j] = -(1 + cal_dis(qpoi[r], j))^0.25 (cw |du[users[r]] - dp[j]|^2 + (1 - cw) |ds[qpoi[r]] - ds[j]|^2)
 * squared distances as float32 differences, the weight in float64 in cal_dis's operation order (Load_Data_prme.py:24-35).  A row with
 * an id out of range is NaN.  poi_prme_score_all writes out (n_rows, n_item); poi_prme_score_topk the k <= 64 (k <= n_item) best ids per
 * row, by descending score then ascending id (poi_score_topk's rule), and their scores when score_out is not NULL; a row with an id out
 * of range gets ids -1.  Timing names: "prme_score_all", "prme_score_topk". */
int poi_prme_score_all(poi_ctx* ctx, const poi_prme_params* prm, const double* coords, const int32_t* users, const int32_t* qpoi, int32_t n_rows,
                       float cw, float* out, void* stream);
int poi_prme_score_topk(poi_ctx* ctx, const poi_prme_params* prm, const double* coords, const int32_t* users, const int32_t* qpoi,
                        int32_t n_rows, float cw, int32_t k, int32_t* idx_out, float* score_out, void* stream);

/* ---- GeoIE (additive to ABI 9) - prog_geoie.py, public/GeoIE.py, public/Load_Data_GeoIE.py -----------------------------------------
 * Tables (GeoIE.py:65-78): g, h, z (n_item + 1, D) with a padding row, t (n_user, D); ab = {a, b} float64 on the device (the launches
 * chain without a host sync).  Float32 tables only; D a multiple of 4, D <= 128 (scoring: [t | m] . [z | h] at width 2 D <= 256). */
typedef struct poi_geoie_params {
  float* g; float* h; float* t; float* z; double* ab;
  int32_t n_user; int32_t n_item; int32_t dim;
} poi_geoie_params;
/* One launch of n users (users[k], rows of the training CSR off / p / q: positions off[u] .. off[u+1]-1 of the flat POIs p and negatives
 * q; coords (n_item, 2) float64 lat, lon; cphi (n_item) = cos(lat * pi / 180), data.cos_lat), replacing GeoIE.seq_train
 * (GeoIE.py:129-188, driver prog_geoie.py:160-185, distances of Load_Data_GeoIE.py:143-156).  For user u with POIs p_0 .. p_{L-1} and
 * negatives q_0 .. q_{L-1}, rows i = 0 .. L-2, columns j <= i:
 *   dp_ij = float32(cal_dis(p_j, p_{i+1})),  dq_ij = float32(cal_dis(p_j, q_{i+1}))  (float64 in cal_dis's operation order),
 *   f(d) = a max(d, d_min)^b (float64),  sp_i - sq_i = (1 / (i + 1)) sum_j (g[p_j].h[p_{i+1}] f(dp_ij) - g[p_j].h[q_{i+1}] f(dq_ij)),
 *   loss_out[k] = sum_i log sigmoid(sp_i - sq_i),  cost = -loss + lambda / 2 (|g[p_0..p_{L-2}]|^2 + |h, z at p_{1..}, q_{1..}|^2)
 * (every gathered occurrence counts); every gathered row moves by -alpha d cost / d row with the user's full accumulated gradient, and
 * a, b by -alpha d cost / d (a, b): t never moves, z by L2 decay only, a and b get no decay.  Undefined cases of the reference (f(0) with
 * b <= 0) follow DESIGN.md section 11: a pair at max(d, d_min) = 0 with b > 0 contributes f = 0 and df/db = 0; a user with an id out of
 * range (users[k] outside [0, n_user), a POI or negative outside [0, n_item)), or with any non-finite value - max(d, d_min) = 0 with
 * b <= 0 included - is REJECTED: it moves nothing (rows, a, b), its loss is NaN, it counts in no k and is counted once
 * (poi_ctx_take_bad_ids).  A user with L < 2 has no rows: loss 0, not counted.  Batch semantics above (poi_ctx_set_batch_cap): every
 * user at the launch-entry values, a row touched by k users moves by min(k, cap) / k times their summed updates, a and b are touched by
 * every accepted user with rows; n == 1 is the reference step.  The 5 touches per row (g[p_i], h and z at p_{i+1}, q_{i+1}) are sorted
 * by (table, row) and summed in a fixed order with no float atomics: identical launches give bitwise identical g, h, z, a, b.
 * n_rows = sum over the launch of max(L - 1, 0), known to the host (scratch is sized from it; no device-to-host sync); a launch whose
 * rows do not add up to it moves nothing and rejects every user.  Timing names: "geoie_plan", "geoie_row", "geoie_col", "geoie_user",
 * "geoie_sort", "geoie_rows", "geoie_commit", "geoie_ab". */
int poi_geoie_step(poi_ctx* ctx, const poi_geoie_params* prm, const int32_t* off, const int32_t* p, const int32_t* q, const double* coords,
                   const double* cphi, const int32_t* users, int32_t n, int64_t n_rows, float alpha, float lambda, double d_min,
                   float* loss_out, void* stream);
/* The float32 dp / dq of a launch (fun_compute_dist_neg, Load_Data_GeoIE.py:143-156, without the zero padding) in packed lower-triangular
 * order: user k (launch order) starts at P_k = sum_{k' < k} R_k' (R_k' + 1) / 2, R = max(L - 1, 0), and its pair (i, j <= i) is at
 * P_k + i (i + 1) / 2 + j.  n_pairs = the host's total.  NaN for a pair with an id out of range, and everywhere when the totals do not
 * match.  Timing name: "geoie_pairs". */
int poi_geoie_pair_distances(poi_ctx* ctx, const int32_t* off, const int32_t* p, const int32_t* q, int32_t n_user, int32_t n_item,
                             const double* coords, const double* cphi, const int32_t* users, int32_t n, int64_t n_rows, int64_t n_pairs,
                             float* dp_out, float* dq_out, void* stream);
/* User side of GeoIE.compute_sub_all_scores (GeoIE.py:117-127): out (n_user, 2 D) row u = [t[u] | m_u], m_u = (sum_{j < L_u} g[p_j]) / nH_u,
 * a float64 sum in sequence order.  norm 0 ("reference"): nH_u = sum_j p_j + (len_max - L_u) n_item, the reference's sum of the padded
 * id row (tra_buys_masks, not the mask); norm 1 ("count"): nH_u = L_u (m_u = 0 for L_u = 0).  Scores s[u, k] = t[u].z[k] + m_u.h[k] then
 * come from poi_score_all / poi_score_topk with items [z | h] at width 2 D.  A POI id outside [0, n_item] makes the row's m NaN.
 * Timing name: "geoie_uvec". */
int poi_geoie_user_vectors(poi_ctx* ctx, const poi_geoie_params* prm, const int32_t* off, const int32_t* p, int32_t n_user, int32_t len_max,
                           int32_t norm, float* out, void* stream);
/* Scoring under the TRAINED rule (additive to 9): the score poi_geoie_step optimises, against every POI.  The
 * reference's scoring (GeoIE.py:117-127, poi_geoie_user_vectors above) drops the power law f; this is its commented-out line
 * `gh = T.sum(gi * hj, 3) * self.f_d(self.trained_f, d) / n_H` without the (n_user, L, n_item) distance list: every distance is recomputed
 * per pair and never stored.  For a history p_0 .. p_{L-1} (ids in [0, n_item)) and a candidate l in [0, n_item):
 *   S(l) = tu . z[l] + (1 / L) sum_{k in distinct(p), ascending id} m_k (g[k] . h[l]) f(d_eff(k, l))
 * m_k = occurrences of k in the history (revisits share one distance: each distinct POI is evaluated once);
 * d = float32(cal_dis(k, l)) exactly as the step computes it (float64, cal_dis's operation order, cphi from the host, no contraction);
 * d_eff = max(d, d_min); f = a exp(b ln d_eff) in float64, the step's arithmetic.  The two D-wide dot products are float32; the sum over
 * k and the user term are accumulated in float64 in a fixed order per (history, candidate); the result is rounded once to float32.  The
 * divisor is L - the step's 1 / (i + 1) with the whole history behind it; score_norm does not apply.  tu (n_rows, D) or NULL (= zero: a
 * user the model never saw; t never moves in training, so a GeoIE user IS its history).
 * Undefined cases (rules 2-4): a pair at d_eff = 0 contributes 0 when b > 0; when b <= 0 the candidate's score is
 * NaN in the matrix, it is never selected by the top-K and counts below every target in poi_rank_scores - this happens exactly when the
 * candidate coincides with a history POI and d_min = 0.  An empty history scores tu . z[l] alone.
 *   off / p / mult  CSR of COMPACTED histories: p the distinct ids of a history in strictly ascending order, mult their multiplicities
 *                   (NULL = 1 each), L = the sum of a row's mult
 *   rows (n_rows)   the histories of the CSR to score, output row r <- history rows[r] (NULL = the identity); trusted like user ids
 *   prm             the tables to score with (the caller's snapshots); t is not read
 * A bad row - off[h + 1] < off[h], an id outside [0, n_item), ids not strictly ascending, a multiplicity < 1, or a malformed exclusion
 * list - gets NaN scores (matrix) or -1 ids, -inf scores and count 0 (top-K), is counted once (poi_ctx_take_bad_ids), and its
 * neighbours are untouched.  The bits of a row depend on its own history, tu and the tables only - not on the other rows of the call,
 * the grid or the span size.  n_rows == 0 is a no-op.
 * poi_geoie_score_all_geo writes out (n_rows, n_item).  Timing name: "geoie_score_geo".
 * poi_geoie_score_topk_geo (1 <= k <= 32): idx_out (n_rows, k) by descending score, ties by ascending id; score_out (n_rows, k) or NULL,
 * bitwise the matrix's values; ex_off (n_rows + 1) / ex per-row exclusion lists under poi_score_topk_near's contract (ids ascending and
 * unique within a row, both NULL = none), skipped before the pair math; count_out (n_rows) or NULL = the selectable candidates of a row
 * (not excluded, score neither NaN nor -inf); a row with fewer than k of them ends in -1 ids and -inf scores.  Timing name:
 * "geoie_topk_geo".
 * Both cut [0, n_item) into spans of "geoie_score_span" candidates (poi_ctx_set_option; 0 = default: about 4 workgroups per CU over the
 * call, at least 256 candidates each; rounded up to a multiple of 16), one workgroup per (row, span); the top-K folds a row's span lists
 * in a second small kernel.  Every span size gives bitwise the same lists and scores.  poi_ctx_last_plan: "geoie_score_span" (the span
 * in force), "geoie_score_splits" (spans per row). */
int poi_geoie_score_all_geo(poi_ctx* ctx, const poi_geoie_params* prm, const int32_t* off, const int32_t* p, const int32_t* mult, const float* tu,
                            const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min, float* out,
                            void* stream);
int poi_geoie_score_topk_geo(poi_ctx* ctx, const poi_geoie_params* prm, const int32_t* off, const int32_t* p, const int32_t* mult, const float* tu,
                             const int32_t* rows, int32_t n_rows, const double* coords, const double* cphi, double d_min, const int32_t* ex_off,
                             const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- POI2Vec (additive to ABI 9) - prog_poi2vec.py, public/POI2Vec.py, public/Load_Data_Poi2vec.py ----------------------------------
 * Tables (POI2Vec.py:63-71): xu (n_user, D), wl (n_item + 1, D) whose last row is the zero pad row wl_m and never moves, pb (n_node, D),
 * float32; D a multiple of 4 in [4, 128].  Tree tables (Load_Data_Poi2vec.py:96-130): routes (n_item + 1, 4, depth) int32 [leaf .. root],
 * lrs (same shape) int8, probs (n_item + 1, 4) float32, row n_item = the pad row (routes[0], lrs[0], probs 0); rid (n_item + 1, 4) int32 =
 * the left-to-right index of each route's leaf (bit d - 1 of it = the child taken at route position d: 0 left, lrs + 1; 1 right,
 * lrs - 1); depth <= 31, the tree is perfect (n_node = 2^depth - 1). */
typedef struct poi_poi2vec_params {
  float* xu; float* wl; float* pb;
  const int32_t* routes; const int8_t* lrs; const float* probs; const int32_t* rid;
  int32_t n_user; int32_t n_item; int32_t n_node; int32_t depth; int32_t dim;
} poi_poi2vec_params;
/* One launch of n users, replacing Poi2vec.seq_train (POI2Vec.py:127-181, driver prog_poi2vec.py:160-164).  Data: CSR of CSR - user u's
 * train positions are off[u] .. off[u+1]-1 of tgt (targets t_i); position x's context POIs are cidx[coff[x] .. coff[x+1]-1] (an id
 * outside [0, n_item) is the reference's padding: it adds the zero row).  For a user with L >= 1 targets:
 *   s_j = xu_u . wl_j (j < n_item),  log plu_j = s_j - logsumexp(s);   c_i = sum_{k in C_i} wl_k,  ind_i = ceil(|mean_d c_i|)
 *   z_ird = pb[routes[t_i][r][d]] . c_i,  S_i = sum_r probs[t_i][r] prod_d (sigmoid(z_ird lrs[t_i][r][d]) ind_i),
 *   paths_i = floor(1 - S_i) + S_i (ceil and floor carry no gradient; both are decided on float64 values),
 *   loss_out[k] = upq = -(1 / L) sum_i (log plu_{t_i} + log paths_i),  cost = upq + lambda / 2 (|xu_u|^2 + |wl|^2)  (nothing on pb).
 * wl moves by -alpha d cost / d wl: DENSE (the softmax term (softmax_j - count_j / L) xu_u and the decay of every row, plus the context
 * term through c_i on the context rows); xu_u by -alpha d cost / d xu_u; pb by the reference's set_subtensor on pb[bidx]: PER OCCURRENCE
 * new = old - alpha d cost / d (that occurrence), assigned in the flattened (i, r, d) order of the bidx padded to len_max, the last write
 * on a node winning.  The padded positions i >= L route through routes[0] and write the old value back last: for a user with
 * L < len_max no node on POI 0's four routes (the root among them) moves.  This is what CPU Theano computes.
 * Batch semantics above (poi_ctx_set_batch_cap): every user at the launch-entry values; wl is touched by every accepted user (k = their
 * number: it moves by min(k, cap) / k times their summed updates), an xu row by its user (k = its accepted occurrences in the launch), a
 * pb row by the users whose collapsed write on it comes from a real position (a padding write is not a touch).  n == 1 at cap 1 is the
 * reference step.  A user with an id out of range (users[k] outside [0, n_user), a target outside [0, n_item)), with L = 0 or with a
 * non-finite loss (paths_i <= 0 included) is REJECTED: it moves nothing, its loss is NaN, it counts in no k and is counted once
 * (poi_ctx_take_bad_ids); removing it from the launch leaves every other result bitwise equal.  No float atomics, every sum in launch
 * order: identical launches give bitwise identical tables.  n_pos / n_ctx = the launch's totals of positions and context entries, known
 * to the host (scratch is sized from them; no device-to-host sync); a launch whose totals do not match moves nothing and rejects every
 * user.  Limits: at most 4096 users per launch; the collapse costs (4 L)^2 integer operations on one workgroup per user and the per-user
 * sums run over L serially, so L is meant to stay within a few thousand; scratch is about 4 bytes x (256 n D + n n_item / 16) + 8 bytes x
 * n_pos (4 depth + 2 D) + 20 bytes x (n_pos 4 depth + n_pos + n_ctx) (256 n D floats of dXU partial sums dominate: 512 MB at n = 4096,
 * D = 128).  Timing names: "p2v_plan", "p2v_lse", "p2v_pos", "p2v_user", "p2v_sort", "p2v_pb", "p2v_dense",
 * "p2v_sparse", "p2v_xu". */
int poi_poi2vec_step(poi_ctx* ctx, const poi_poi2vec_params* prm, const int32_t* off, const int32_t* tgt, const int32_t* coff,
                     const int32_t* cidx, const int32_t* users, int32_t n, int64_t n_pos, int64_t n_ctx, int32_t len_max, float alpha,
                     float lambda, float* loss_out, void* stream);
/* Poi2vecBasic.compute_sub_all_scores (POI2Vec.py:91-109) in factorised form.  Rows (user b, position t), b < n_batch, t < length, row
 * r = b length + t with the explicit context row coff[r] .. coff[r+1]-1 of cidx (the caller picks the reference's train-table rows or
 * the test contexts).  Per row: cl = sum of wl over the context; z_n = pb_n . cl for every node ONCE (float64), f = sigmoid(z_n lr)
 * ceil(|z_n|); the product of f along each of the 2^(depth-1) distinct routes (leaf_nodes (n_leaf, depth) int32 [leaf .. root] of the
 * leaf with left-to-right index l; lr from the bits of l); S_j = sum_r probs[j][r] product[rid[j][r]]; paths_j = floor(1 - S_j) + S_j;
 * out[r][j] = paths_j plu[b][j], j < n_item, where plu = softmax of xu[users] . wl^T over the USERS of the batch (softmax_axis 0, the
 * reference: POI2Vec.py:92, 183-186) or over the POIs (softmax_axis 1).  prm->xu / wl / pb are the snapshots to score.  A user id out of
 * range gives NaN rows for that user only (its logits are left out of the softmax over the users).  Scratch: rows (n_node + n_leaf + D)
 * float64 values + n_batch n_item floats.  Timing names: "p2v_sc_node", "p2v_sc_route", "p2v_sc_plu", "p2v_sc_out". */
int poi_poi2vec_scores(poi_ctx* ctx, const poi_poi2vec_params* prm, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch,
                       int32_t length, const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, float* out, void* stream);
/* The same scores reduced to the top k per row (k <= 64), fused into the score pass: a workgroup per row computes the scores on the fly
 * (the row of scores is never stored) and keeps sorted candidate lists in LDS.  idx_out (rows, k) int32 by descending score, ties by
 * ascending id, NaN scores last; score_out (rows, k) or NULL, bitwise the values poi_poi2vec_scores writes.  Timing name: "p2v_sc_topk"
 * (in place of "p2v_sc_out"). */
int poi_poi2vec_topk(poi_ctx* ctx, const poi_poi2vec_params* prm, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch,
                     int32_t length, const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, int32_t k, int32_t* idx_out,
                     float* score_out, void* stream);

/* poi_poi2vec_topk with per-row exclusion lists (additive to 9): ex_off (rows + 1) / ex are a CSR of ascending unique POI ids per output
 * row (the contract of poi_score_topk_near's lists), or both NULL.  An excluded POI is never listed.  count_out (rows) or NULL: the
 * number of POIs ranked, n_item minus the row's excluded ids.  A row with fewer than k candidates ends in id -1 with a NaN score (an empty
 * list slot).  With ex_off = ex = count_out = NULL the call is poi_poi2vec_topk: the same bits. */
int poi_poi2vec_topk_ex(poi_ctx* ctx, const poi_poi2vec_params* prm, const int32_t* leaf_nodes, const int32_t* users, int32_t n_batch,
                        int32_t length, const int32_t* coff, const int32_t* cidx, int32_t softmax_axis, const int32_t* ex_off,
                        const int32_t* ex, int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- fold-in for POI2Vec (additive to 9): a row of xu for a check-in history the model never trained on ------------------------------------
 * In Poi2vec.seq_train (public/POI2Vec.py:140-163) the geographic factor paths_i depends on wl, pb and the contexts, never on xu.  With
 * the item side frozen the user row sees only the full softmax over all POIs.  For new user r with history t_i = tgt[off[r] .. off[r+1]),
 * L = its length:
 *   w = w0[r] (zeros when w0 is NULL);  for e = 0 .. epochs - 1:
 *     s_j = w . wl_j  (j < n_item),   lse = logsumexp_j s_j,   plu = softmax_j s_j,
 *     loss[r][e] = lse - (1/L) sum_i s_{t_i}                                     (at the values before the update),
 *     w = w - alpha (sum_j plu_j wl_j - (1/L) sum_i wl_{t_i} + lambda w)         (one step per pass over the history)
 *   This is the xu[u] part of poi_poi2vec_step for one user: from w0 = xu[u], one epoch gives that step's xu[u]; the loss is the
 *   step's upq minus its mean log paths term, which does not depend on w.
 *   wl: the evaluation snapshot, float32, at least n_item rows; the softmax runs over rows 0 .. n_item - 1 only - the zero pad row
 *   n_item never enters it.  Ids lie in [0, n_item): the pad id is not a POI of the softmax and is rejected, as poi_poi2vec_step does.
 *   A repeated target counts as often as it occurs.
 * Arithmetic: the running w, the logits, the exponentials, every sum and the loss are float64 (alpha and lambda are taken at their
 * float values); w is rounded to float32 once, at the end.  Every exponential has a running maximum subtracted: any finite w0 gives
 * finite rows and losses.  No float atomics; partials are formed per span of P2V_FOLD_SPAN = poi_foldin_p2v_span() items and merged
 * in span order.  A user's output bits depend on its own history and w0 alone: not on the other users of the call, on its position in
 * the call, on n or on the grid.
 * Edge cases: epochs = 0 or an empty history returns w0[r] (zeros without w0) and losses 0.  A user with off[r + 1] < off[r],
 * off[r] < 0 or a target outside [0, n_item) is a bad user: a NaN row, NaN losses, counted once (poi_ctx_take_bad_ids), and nothing
 * else moves.  The offsets themselves must lie inside tgt (the caller's contract).  n = 0 is a no-op.
 * w_out (n, dim) may alias w0; loss_out (n, epochs) or NULL.  dim: a multiple of 4 in [4, 128].
 * Scratch: 8 bytes x c (n_span (dim + 2) + 2 dim) + 4 c, n_span = ceil(n_item / span), for c = the users of a chunk: the call is cut
 * into chunks of c = max(64, 64 MiB / (8 n_span (dim + 2)) rounded down to a multiple of 64) users, which changes no bit.
 * Per epoch two kernels (foldin_p2v.hip): a pass over wl (16 users x 16 POIs per v_mfma_f64_16x16x4_f64 block, item tiles staged in
 * LDS as float64) and a combine-and-update.  Timing names: "foldin_p2v_prep", "foldin_p2v_pass", "foldin_p2v_upd". */
int poi_foldin_p2v(poi_ctx* ctx, const float* wl, int32_t n_item, int32_t dim, const int32_t* off, const int32_t* tgt, int32_t n,
                   int32_t epochs, float alpha, float lambda, const float* w0, float* w_out, float* loss_out, void* stream);
int poi_foldin_p2v_span(void);      /* the span of the partials (a compile-time constant; tests straddle it) */

/* ---- mini-batch Lstm / Rnn (additive to ABI 9) - public/GRU.py:502-657 (Lstm), :661-809 (Rnn) ---------------------------------------
 * The baselines the reference's papers compare against, as one kernel family templated on the number of gate blocks.  lt (n_item + 1, D);
 * Lstm: ui, wh (4, D, D), bi (4, D), gates i, f, g, o (GRU.py:562-567); Rnn: ui, wh (D, D), bi (D), h = sigmoid(ui x + wh h + bi)
 * (:720-722).  h0 = c0 = 0, never trained.  Float32 tables only; D a multiple of 4 up to 256 at its native width.
 * poi_cell_step replaces seq_train(start_end) (GRU.py:525-605, :682-760): the launch is ONE mini-batch of n_seq users - the rule
 * poi_ctx_set_batch_cap(0) documents for `Gru`, always (the batch cap is ignored):
 *   u_t = h_{t-1} . (lt[p_t] - lt[q_t]), t = 0 .. L-1;  out[k] = -sum_t log sigmoid(u_t)  (the reference returns their sum, :600)
 *   cost = sum_k out[k] / n + lambda / 2 (|lt[p]|^2 + |lt[q]|^2 over all n x len_max gathered positions, pad rows and duplicates
 *          counted, + |ui|^2 + |wh|^2 + |bi|^2)                                          (:582-588, :737-743)
 *   dense: theta -= alpha (G / n + lambda theta);  every row of unique(p U q): row -= alpha (G_row / n + lambda mult row), mult = its
 *   count over all len_max positions of all n users (the pad row n_item included), every right-hand side at the launch-entry values.
 * A user runs exactly L-1 cell steps: the reference scans to the batch's longest L and feeds pad rows to shorter users, but those steps
 * carry no loss and nothing reads them.  Float64 gate sums, states, BPTT and gradient sums, rounded once at the write-back; alpha /
 * lambda as their shortest decimals (engine 4's rule).  No float atomics: the row touches are sorted and summed in a fixed order and
 * the dense gradients are chunk partials added in chunk order - identical launches give bitwise identical tables, on any grid.
 * A launch with a user id outside [0, n_user), a POI or negative outside [0, n_item] or a length outside [1, max_len] moves NOTHING:
 * the offending users' losses are NaN and they are counted (poi_ctx_take_bad_ids).  Scratch grows with n_seq x max_len position rows
 * (8 (G + 3) D + 8 D bytes each).  Timing names: "cell_plan", "cell_rec", "cell_wgrad", "cell_sort", "cell_rows", "cell_commit".
 * poi_cell_predict replaces seq_predict(start_end) (:610-657, :765-809): the cell over all L positions of the snapshot prm->lt,
 * hts (n, D) row out_row[k] (or k when out_row is NULL) = h_{L-1} of uidx[k]; a user with an id out of range gets a NaN row and is
 * counted.  Timing name: "cell_predict". */
enum { POI_CELL_RNN = 1, POI_CELL_LSTM = 4 };            /* = number of gate blocks */
typedef struct poi_cell_params { float* lt; float* ui; float* wh; float* bi; int32_t n_item; int32_t dim; int32_t cell; } poi_cell_params;
int poi_cell_step(poi_ctx* ctx, const poi_cell_params* prm, const poi_seq_tables* tab, const int32_t* uidx, int32_t n_seq,
                  float alpha, float lambda, float* out /* n_seq: -sum_t log sigmoid(u_t) per user */, void* stream);
int poi_cell_predict(poi_ctx* ctx, const poi_cell_params* prm, const poi_seq_tables* tab, const int32_t* uidx, const int32_t* out_row,
                     int32_t n, float* hts, void* stream);   /* prm->lt = the snapshot */

/* ---- VBPR (additive to ABI 9) - OboVBpr, public/BPR.py:245-335 ------------------------------------------------------------------------
 * BPR-MF with a fixed per-item feature table and a trained dense projection.  Float32 tables on the device: ux, ue (n_user, D);
 * lt (n_item + 1, D); ei (D, F); fi (n_item + 1, F), never written, row n_item the (zero) pad row.  D = dim a multiple of 4 up to 128,
 * F = n_img a multiple of 4 up to 4096, every table 16-byte aligned (else POI_ENOTSUP / POI_EINVAL).
 * poi_vbpr_step replaces bpr_train(uidx, [p, q]) (:268-319) for n triples, every right-hand side at the launch-entry values:
 *   d = fi[p] - fi[q];  v = ei d;  x = ux[u] . (lt[p] - lt[q]) + ue[u] . v;  g = -sigmoid(-x);  loss_out[i] = -log sigmoid(x)
 *   ux[u] -= alpha (g (lt[p] - lt[q]) + lambda ux[u])      ue[u] -= alpha (g v + lambda ue[u])
 *   lt[p] -= alpha (g ux[u] + lambda lt[p])                lt[q] -= alpha (-g ux[u] + lambda lt[q])
 *   ei    -= alpha (g ue[u] (x) d + lambda_ev ei)
 * Launches of n > 1 triples follow "Batch semantics" above: a row of ux / ue / lt touched by k triples moves by min(k, cap) / k of their
 * summed updates; ei, touched by all n_acc accepted triples, by min(n_acc, cap) / n_acc of -alpha (sum_i g_i ue[u_i] (x) d_i + n_acc
 * lambda_ev ei).  n == 1 is the reference step for every cap; batch cap 0: POI_ENOTSUP.
 * Arithmetic: both matrix products over the gathered differences - V = Dmat ei^T and d ei = G^T Dmat - run on the FLOAT64 matrix cores
 * (v_mfma_f64_16x16x4_f64) from the float32 tables, as do x, g, the loss and the ei step; the row sums of ux / ue / lt are float32.  The
 * n x F difference matrix is never stored; a triple's two feature rows are read twice per step.  No float atomics: the 4 n row touches
 * are sorted by (table, row) and summed run by run; d ei is summed as row-chunk partials over the ACCEPTED triples in launch order (at
 * most 64 chunks of 64 ceil(ceil(n / 64) / 64) triples: a function of n alone) added in chunk order.  Identical launches give bitwise
 * identical tables on any grid ("vbpr_grid").
 * Bad ids: a triple with u outside [0, n_user), p or q outside [0, n_item], or p == q moves nothing, has loss NaN and is counted once
 * (poi_ctx_take_bad_ids).  Removing it from the launch leaves every row of ux / ue / lt and every loss bitwise equal, and ei too whenever
 * both launches have the same chunk length (always up to 4096 triples).
 * Scratch (context-owned, grows with the launch): 8 n_chunk D F + 20 n D + ~60 n bytes.  No device-to-host sync inside a launch.
 * Timing names: "vbpr_fwd", "vbpr_wgrad", "vbpr_sort", "vbpr_rows", "vbpr_commit".
 * poi_vbpr_items (update_trained_items, :321-329): items_out (n_item + 1, 2 D) = [lt | fi ei^T], the product on the same MFMA written
 * straight into the right half.  Timing name: "vbpr_items".
 * poi_vbpr_users (:331-335): users_out (n_user, 2 D) = [ux | ue].  Timing name: "vbpr_users".
 * Scoring, top-K and AUC on the two outputs: poi_score_all / poi_score_topk / poi_auc_preference with dim = 2 D. */
typedef struct poi_vbpr_params {
  float* ux; float* lt; float* ue; float* ei; const float* fi;
  int32_t n_user; int32_t n_item; int32_t dim; int32_t n_img;
} poi_vbpr_params;
int poi_vbpr_step(poi_ctx* ctx, const poi_vbpr_params* prm, const int32_t* uidx, const int32_t* p, const int32_t* q, int32_t n, float alpha,
                  float lambda, float lambda_ev, float* loss_out /* n */, void* stream);
int poi_vbpr_items(poi_ctx* ctx, const poi_vbpr_params* prm, float* items_out, void* stream);
int poi_vbpr_users(poi_ctx* ctx, const poi_vbpr_params* prm, float* users_out, void* stream);

/* ---- online sessions (additive to 9; new - the reference can only rerun whole training sequences) ----------------------------------
 * Per-slot recurrent state of the GRU family (OboSpatialGru, OboGru, Gru: one cell) kept on the device and advanced ONE check-in at a
 * time.  State of slot s, owned by the caller: h (n_slot, D) FLOAT64 (one rounding less per step than a float32 state; 8 D bytes per
 * slot), sts (n_slot, n_dist + 1) float32 (spatial only), last_poi (n_slot) int32 with -1 = no check-in yet, steps (n_slot) int32.
 * poi_session_advance applies n events (slot[i], poi[i]) - the cell step of seq_predict (public/GRU_Spatial.py:231-288,
 * public/GRU.py:154-202) on the snapshots prm->lt / prm->di:
 *   d      = n_dist if last_poi[s] < 0, else bin(coords[j], coords[last_poi[s]])  (data.dist_pos_bins: same argument order, cphi / thr)
 *   x      = [lt[j] | di[d]]  (spatial)  or  lt[j]  (plain: prm->di / vs / bs NULL, n_dist 0; coords / cphi / thr / sts may be NULL)
 *   z, r   = sigmoid(ui[0:2] x + wh[0:2] h + bi[0:2]);  c = tanh(ui[2] x + wh[2] (r * h) + bi[2])
 *   h[s]   = (1 - z) * h + z * c;  last_poi[s] = j;  steps[s] += 1;  sts[s] = softmax(vs h[s] + bs)  (spatial)
 * so a zeroed slot (h = 0, last_poi = -1) advanced through p[0 .. L-1] holds what poi_gru_predict returns for that training row.
 * The update is in place; hts_out (n, D) / sts_out (n, n_dist + 1) are optional float32 copies of the new rows.  dd in metres.
 * Tables are float32, the POI snapshot may be a registered half table; a half di, or more than 4095 bins: POI_ENOTSUP.  Products,
 * gate sums and the softmax are float64.  No atomics touch a result and every sum has a fixed order: identical calls give bitwise
 * identical state.
 * Repeated slots: a slot named by MORE THAN ONE event of a call is refused - every event of it is treated as a bad id - because
 * the events of a call run concurrently.  Split such a batch into successive calls that keep each slot's order (models.Session.advance).
 * Bad ids: a slot outside [0, n_slot) or a POI outside [0, n_item) leaves the state untouched, gives NaN rows in hts_out / sts_out
 * and is counted (poi_ctx_take_bad_ids).
 * Two launch regimes: below "session_tile_min" events (poi_ctx_set_option, default 512) one workgroup per event streams the weights
 * from L2 (latency bound: live traffic); from there on 16 events per workgroup run on the float64 matrix cores (replay / bulk; needs
 * D % 16 == 0 and the tile's LDS, else the event path serves every size).  poi_ctx_last_plan: "session_path" (0 event, 1 tile),
 * "session_tiles" (workgroups of the tile kernel, 0 on the event path), "session_tile_min" (the switch point in force).
 * Timing names: "session_advance", "session_sts".
 * poi_session_sts: the head alone - sts_out (n, n_dist + 1) row i = softmax(vs h[slot[i]] + bs), for state seeded from outside
 * (poi_gru_predict rows, a checkpoint); a slot out of range gives a NaN row and is counted. */
int poi_session_advance(poi_ctx* ctx, const poi_gru_params* prm, const double* coords, const double* cphi, const double* thr, double dd,
                        double* h, float* sts, int32_t* last_poi, int32_t* steps, int32_t n_slot, const int32_t* slot,
                        const int32_t* poi, int32_t n, float* hts_out, float* sts_out, void* stream);
int poi_session_sts(poi_ctx* ctx, const poi_gru_params* prm, const double* h, int32_t n_slot, const int32_t* slot, int32_t n,
                    float* sts_out, void* stream);

/* ---- leave-one-out attribution (additive to 9) ----------------------------------------------------------------------------------------
 * WHY was POI j recommended: the score of j under the row's whole history minus its score with one check-in (or every visit of one
 * POI) taken out.  prm / coords / cphi / thr / dd as poi_session_advance takes them (the evaluation snapshots; prm->wd is read by the
 * spatial model).  Row r of n has the history h_ids[h_off[r] .. h_off[r + 1]) (total ids in all) and the list lists[r][0 .. n_list),
 * n_list <= 32, -1 = no entry.  grp[t] is the GROUP of position t within its row (one per check-in: its index; one per distinct POI:
 * the POI's rank by first occurrence); row r has the groups 0 .. g_off[r + 1] - g_off[r] - 1, and group g of row r is row
 * g_off[r] + g of delta (n_group rows in all).
 *   A VARIANT is the history without the positions of one group.  Its state is what a fresh poi_session_advance slot holds after the
 * kept positions in order: the step after a removed check-in is binned against the last KEPT POI (n_dist without one), last_poi is
 * the last kept POI (-1 without one), sts = softmax(vs h + bs).  score(v, j) = h_v . lt[j] + wd sts_v[bin(last_v, j)] (the term only
 * for bins below n_dist and last_v >= 0, spatial only).  State, head, softmax and the dot product over the float32 / half row are
 * float64.  base[r][c] = score(whole history, lists[r][c]); delta[g_off[r] + g][c] = base[r][c] - score(variant g, lists[r][c]):
 * positive - the check-in pushed the POI up.  A -1 entry gives NaN in both.  A row without history has no variant; its base is the
 * score of h = 0 without the distance term.  Optional h_out (n_group, dim), sts_out (n_group, n_dist + 1), last_out (n_group): the
 * state of every variant.
 *   Columns.  One persistent kernel walks 16 COLUMNS per workgroup with their states in LDS for all steps; a column is an int32
 * quadruple (row, key, start, 0).  base_cols: n of them, key -1, one per row - walked first, they write base and keep h after every
 * 16th position in a context workspace (n x floor((max_len - 1) / 16) x dim float64; max_len >= the longest history).  var_cols:
 * n_var of them, key = the group removed, start = 16 floor(f / 16) for a group that first occurs at position f: the column starts
 * there from the checkpoint (option "explain_start" 0: every column at 0 from h = 0 - the same bits).  Order both longest remaining
 * walk first; columns of different rows share a workgroup.  A column outside these rules writes nothing.  The bits of a column do
 * not depend on its workgroup, its neighbours or the start mode.
 *   dim must be a multiple of 16 in [16, 256] (the shapes of the session tile kernel; every pad_dim model) - POI_ENOTSUP otherwise.
 * A row with a history POI outside [0, n_item), a listed id outside [-1, n_item) or offsets outside [0, total] gives NaN in base, its
 * deltas and its states and is counted once (poi_ctx_take_bad_ids).  poi_ctx_last_plan: "explain_columns", "explain_tiles",
 * "explain_start".  Timing names: "explain_base", "explain_walk". */
int poi_explain_loo(poi_ctx* ctx, const poi_gru_params* prm, const double* coords, const double* cphi, const double* thr, double dd,
                    const int32_t* h_off, const int32_t* h_ids, int64_t total, const int32_t* grp, const int32_t* g_off, int32_t n_group,
                    int32_t n, int32_t max_len, const int32_t* base_cols, const int32_t* var_cols, int32_t n_var, const int32_t* lists,
                    int32_t n_list, double* base, double* delta, double* h_out, double* sts_out, int32_t* last_out, void* stream);

/* ---- online sessions of the baselines Lstm / Rnn / CA-RNN (additive to 9) ------------------------------------------------------------
 * The same per-slot state, owned by the caller, for the three recurrent classes poi_session_advance does not cover: h (n_slot, D)
 * FLOAT64, c (n_slot, D) FLOAT64 (the Lstm's cell state; NULL for POI_CELL_RNN), last_poi (n_slot) int32 with -1 = no check-in yet,
 * steps (n_slot) int32.  There is no sts.  Both entries apply n events (slot[i], poi[i]) with j = poi[i], s = slot[i]; they are the cell
 * steps of poi_cell_predict / poi_carnn_predict on the snapshots prm->lt (and prm->wd), so a zeroed slot (h = c = 0, last_poi = -1)
 * advanced through p[0 .. L-1] holds what those entries return for that training row.
 * poi_session_cell_advance (prm->cell = POI_CELL_RNN | POI_CELL_LSTM; public/GRU.py:720-722 and :562-567):
 *   Rnn    h[s] = sigmoid(ui lt[j] + wh h[s] + bi)
 *   Lstm   a = ui lt[j] + wh h[s] + bi  (four blocks of D rows);  i, f, o = sigmoid(a0), sigmoid(a1), sigmoid(a3);  g = tanh(a2)
 *          c[s] = f * c[s] + i * g;  h[s] = o * tanh(c[s])
 * poi_session_carnn_advance (public/CA_RNN.py:172-217, literally - the predict graph adds-then-sums):
 *   d      = n_dist if last_poi[s] < 0, else bin(coords[j], coords[last_poi[s]])  (data.dist_pos_bins: the argument order, cphi and thr
 *            of poi_session_advance; dd in metres)
 *   h[s]   = sigmoid(M lt[j] + rowsum(wd[d]) + sum(h[s]))  with rowsum = the sum over the last axis of the (D, D) matrix wd[d] and
 *            sum(h[s]) the scalar sum of the previous state
 * All three: last_poi[s] = j; steps[s] += 1; the update is in place; hts_out (n, D) is an optional float32 copy of the new h rows.
 * Precision: tables are float32 at the model's own dim (these classes are never stored padded; a registered half table: POI_ENOTSUP);
 * every product, gate sum, sigmoid and tanh is float64.  No atomics touch a result and every sum has one fixed order: identical calls
 * give bitwise identical state.  dim must be a multiple of 4 in [4, 256] - what poi_cell_predict and poi_carnn_predict accept - else
 * POI_ENOTSUP; no row is read past its end.
 * Repeated slots and bad ids: exactly as poi_session_advance - a slot named by more than one event of a call, a slot outside
 * [0, n_slot) or a POI outside [0, n_item) leaves the state untouched, gives a NaN row in hts_out and is counted
 * (poi_ctx_take_bad_ids).  Split a batch that repeats slots into successive calls (models.CellSession.advance does).
 * Launch regimes: below "session_tile_min" events (default 512) one workgroup per event streams the weights from L2 - per event
 * 8 D^2 bytes for Rnn and CA-RNN (ui + wh, or M + wd[d]), 32 D^2 for Lstm; from there on, with D % 16 == 0, 16 events per workgroup
 * run on the float64 matrix cores and read the weights once per tile (CA-RNN: the row sums of all n_dist + 1 matrices are rewritten
 * into context scratch by a pre-pass of every such call, so the entry follows a changed prm->wd without a cache).  Otherwise the event
 * path serves every size.  poi_ctx_last_plan: "session_path", "session_tiles", "session_tile_min" as poi_session_advance writes them.
 * Timing names: "session_cell_advance", "session_carnn_advance". */
int poi_session_cell_advance(poi_ctx* ctx, const poi_cell_params* prm, double* h, double* c, int32_t* last_poi, int32_t* steps,
                             int32_t n_slot, const int32_t* slot, const int32_t* poi, int32_t n, float* hts_out, void* stream);
int poi_session_carnn_advance(poi_ctx* ctx, const poi_carnn_params* prm, const double* coords, const double* cphi, const double* thr,
                              double dd, double* h, int32_t* last_poi, int32_t* steps, int32_t n_slot, const int32_t* slot,
                              const int32_t* poi, int32_t n, float* hts_out, void* stream);

/* ---- restricted recommendation (additive to 9): top-K within a radius of an anchor POI, skipping listed POIs ---------------------------
 * public/Valuate.py:132-146 ranks over every POI; FPMC-LR defines its candidates as the POIs within UD km of the last check-in
 * (public/Load_Data_fpmc_lr.py:114-143).  This entry ranks over
 *   C(r) = { j in [0, n_item) : (anchor[r] < 0 or c(anchor[r], j) < c_r or j == anchor[r]) and j not in ex[ex_off[r] .. ex_off[r + 1]) }
 * only: it gathers the candidates' item rows, applies the score rule below and keeps a top-K.
 *   c        the float64 Haversine term in cal_dis's operation order from coords / cphi, exactly as poi_fpmc_neighbor_* and poi_dist_prob
 *            evaluate it; c_r = data.ud_threshold(r km), so that c < c_r <=> dist <= r km.  c_r = +inf, or anchor[r] == -1, means no
 *            radius test for the call or the row.  The anchor itself is a candidate unless it is excluded.
 *   band     lat_order = the stable argsort of latitude that the FPMC-LR neighbour entries take; a row with a radius walks only the
 *            latitude band that can hold candidates (a conservative superset - the exact test alone decides).
 *   ex       per-row exclusion lists: ex_off (n + 1) ascending offsets into ex, ids ascending and unique within a row; both NULL = none.
 *   score    users[r] . items[j] in float32, one fixed summation order per pair that does not depend on how the band is cut; with
 *            wd / sts / thr non-NULL plus wd * sts[r][bin] for bin < n_dist, the bin from the same c through thr (data.bin_thresholds, dd
 *            in metres) - the rule of poi_score_topk_geo.  A row with anchor[r] == -1 has no distance term.  sts is (n, n_dist + 1) and is
 *            read for exactly n rows.  items may be a registered half table; rows >= n_item (the padding row) are never read.
 *   outputs  idx_out (n, k), k <= 32, by descending score, ties by ascending id; a row with fewer than k candidates is filled with -1 ids
 *            and -inf scores (score_out (n, k) or NULL); count_out (n) or NULL = |C(r)|, not clipped to k.
 *   bad rows an anchor outside [-1, n_item) or an exclusion id outside [0, n_item): the row is all -1 / -inf / count 0 and is counted
 *            (poi_ctx_take_bad_ids).
 * coords / cphi / anchor may be NULL when there is neither a radius nor a distance term, lat_order when there is no radius.
 * dim: a multiple of 4, up to 256.  No float atomics: identical calls give bitwise identical outputs, and so do different grids.
 * Two launch regimes: calls of at most "near_split_max" rows (poi_ctx_set_option, default 256: live traffic) cut each row's band into
 * slices, one workgroup each, and merge the slices' lists in a second kernel; larger calls run one workgroup per row.
 * poi_ctx_last_plan: "near_path" (0 row, 1 split), "near_splits" (slices per row, 0 on the row path), "near_split_max" (the switch point
 * in force).  Timing name: "score_topk_near". */
int poi_score_topk_near(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                        const double* coords, const double* cphi, const int32_t* lat_order, const int32_t* anchor, double c_r,
                        const int32_t* ex_off, const int32_t* ex,
                        const float* wd, const float* sts, const double* thr, int32_t n_dist, double dd,
                        int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- exact target ranks (additive to 9): where given POIs stand among ALL POIs ------------------------------------------------------------
 * public/Valuate.py knows a held-out POI only through a top-K list (:132-146) or one sampled negative (:113-118).  These entries give
 * its exact rank, from which MRR, mean / median rank, recall at any cut-off and the AUC over all negatives follow, without an
 * (n, n_item) score matrix.
 *   C(r)            = [0, n_item) minus ex[ex_off[r] .. ex_off[r + 1])
 *   rank_out[r][i]  = |{ j in C(r), j != t : s(r, j) > s(r, t) or (s(r, j) == s(r, t) and j < t) }|   for t = tgt[r][i], tmask[r][i] != 0,
 *                     t in C(r): the tie rule of every top-K entry, i.e. the 0-based position of t in an endless poi_score_topk list.
 *   count_out[r]    = |C(r)| (n), or NULL.
 *   -1              for a masked position (tmask 0: tgt is not read as an id), for an excluded target, and for a target outside
 *                   [0, n_item), which is also counted (poi_ctx_take_bad_ids).
 *   s(r, j)         users[r] . items[j] in float32 on the f32 matrix pipe (exact products, one fixed k order); with wd non-NULL plus
 *                   wd * sts[r][bin(last_poi[r], j)] for bin < n_dist - the arguments and the rule of poi_score_topk_geo (sts (n, n_dist + 1)
 *                   is read for exactly n rows).  wd NULL: the plain score; sts / coords / cphi / thr / last_poi are then ignored.
 *                   A target's own score comes from the same product routine and k order as the streamed scores, so a POI whose item row
 *                   equals the target's ties bit for bit and the index decides.  score_out (n, len_t) or NULL: s(r, t), -inf where the
 *                   rank is -1.
 *   tgt, tmask      (n, len_t) int32, 1 <= len_t <= 8 (larger: POI_ENOTSUP).
 *   ex              as poi_score_topk_near: ex_off (n + 1) ascending offsets into ex, ids ascending and unique within a row, both NULL =
 *                   none.  A row whose list is not ascending or leaves [0, n_item) is rejected: ranks -1, count 0, counted once.
 *   items           float32 or a registered half table; rows >= n_item (the padding row) are never read.  dim: a multiple of 4, <= 256.
 * Two kernels: the targets' scores (which also set rank_out to 0 / -1), then the tile walk of the fused top-K with a compare-and-count
 * epilogue; the item range of a 32-row tile is split over up to "rank_grid" wavefronts and every (row, target) receives integer
 * atomic adds only - identical calls and different grids give identical ranks.  poi_ctx_last_plan "rank_splits": the split taken.
 * Timing name: "score_rank".  n = 0 is a no-op. */
int poi_score_rank(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                   const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                   int32_t n_dist, double dd,
                   const int32_t* tgt, const int32_t* tmask, int32_t len_t, const int32_t* ex_off, const int32_t* ex,
                   int32_t* rank_out, float* score_out, int32_t* count_out, void* stream);
/* The same definition on explicit score rows scores (n, n_item) - the counterpart of poi_topk for models whose score is not
 * users . items, and an independent check of the counting.  NaN scores count as below every target.  Timing name: "rank_scores". */
int poi_rank_scores(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, const int32_t* tgt, const int32_t* tmask, int32_t len_t,
                    const int32_t* ex_off, const int32_t* ex, int32_t* rank_out, int32_t* count_out, void* stream);

/* ---- group recommendation (additive to 9): the top-K of an aggregate of the members' scores, for a party of users -----------------------
 * Every other ranking entry answers for one user row.  A party - friends choosing a place, a family on a trip - is ranked by an
 * aggregate of its members' scores, which is not the score of any single row: the minimum is not linear, and under the distance term
 * every member stands at a last POI of their own.  These entries rank n_grp groups without the (members, n_item) score matrix.
 *   users, g_off, g_mem   n member rows users (n, dim); the groups as a CSR: g_off (n_grp + 1) ascending offsets into g_mem, g_mem row
 *                         indices into users.  A row listed twice counts twice.
 *   s(m, j)               exactly poi_score_rank's s(r, j): users[m] . items[j] in float32 from the same product routine and k order
 *                         (f32 matrix pipe, exact products); with wd non-NULL plus wd * sts[m][bin(last_poi[m], j)] for bin < n_dist - the
 *                         arguments and the rule of poi_score_topk_geo (sts (n, n_dist + 1)).  A member with last_poi[m] < 0 has no distance
 *                         term.  wd NULL: the plain score; sts / coords / cphi / thr / last_poi are then ignored.
 *   a(g, j), agg = 1      least misery: the minimum of s(m, j) over the group's list.  Exact: permuting the list changes no bit of the
 *                         output (a zero comes out as +0 whichever sign the members' zeros have).
 *   a(g, j), agg = 0      mean: the float32 sum of s(m, j) over the list divided by float(M), one IEEE division.  ORDER OF THE ADDITIONS: a
 *                         left-to-right chain in list order, ((s(m_0) + s(m_1)) + s(m_2)) + ... - a function of the members' positions in
 *                         the group's list alone, not of the grid, of how the item range is cut, of the group's place in the call or of
 *                         the other groups.
 *   NaN                   a POI for which any member's score is NaN is never selected.
 *   C(g)                  [0, n_item) minus ex[ex_off[g] .. ex_off[g + 1]): ONE exclusion list per group, the conventions of
 *                         poi_score_topk_near (ascending unique ids; both pointers NULL = none).
 *   outputs               idx_out (n_grp, k), k <= 32, by descending a, ties by ascending id; -1 ids and -inf scores where |C(g)| < k;
 *                         score_out (n_grp, k) or NULL; count_out (n_grp) or NULL = |C(g)|.
 *   bad groups            a member outside [0, n), descending g_off, an exclusion id outside [0, n_item) or a list that is not ascending:
 *                         the group is all -1 / -inf / count 0 and is counted once (poi_ctx_take_bad_ids).
 *   empty group           all -1 / -inf, count 0, not counted.  n_grp = 0 is a no-op.  Any group size: a list longer than the 32 rows of a
 *                         tile is walked in chunks and the aggregate carried from chunk to chunk.
 *   items                 float32 or a registered half table; rows >= n_item (the padding row) are never read.  dim: a multiple of 4, <= 256.
 * No float atomics: identical calls give bitwise identical outputs, every grid and split gives the same outputs as every other, and a
 * group gives the same outputs alone as inside a larger call.
 * Two launch regimes: calls of at most "group_split_max" groups (poi_ctx_set_option, default 256: live traffic, often one party) cut
 * the item range into "group_grid" slices, one workgroup each, and merge the slices' lists in a second kernel; larger calls run one
 * workgroup per 8 groups, which it packs whole into passes of at most 32 member rows.  poi_ctx_last_plan: "group_path" (0 tile, 1 split),
 * "group_splits" (slices, 0 on the tile path), "group_split_max" (the switch point in force).  Timing name: "group_topk". */
int poi_group_topk(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                   const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                   int32_t n_dist, double dd,
                   const int32_t* g_off, const int32_t* g_mem, int32_t n_grp, int32_t agg, const int32_t* ex_off, const int32_t* ex,
                   int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);
/* The same definition on explicit score rows scores (n, n_item), g_mem indexing its rows - to poi_group_topk what poi_rank_scores is to
 * poi_score_rank: for the models whose score is not users . items, and an independent check of the aggregation and the selection.
 * One workgroup per group.  Timing name: "group_topk_scores". */
int poi_group_topk_scores(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item,
                          const int32_t* g_off, const int32_t* g_mem, int32_t n_grp, int32_t agg, const int32_t* ex_off, const int32_t* ex,
                          int32_t k, int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- route recommendation (additive to 9): beam search over a session's next N POIs ---------------------------------------------------------
 * Every other serving entry stops at one hop: the best next place for a state that exists.  A route - "plan my afternoon" - is not the
 * top-N of one ranking: the second stop depends on the first, the recurrent state moves, and under the distance term the next hop is
 * measured from the stop before it.  These two entries are one step of a beam search; the state gathering between steps is the caller's
 * (index_select) and the advance is poi_session_advance / poi_session_cell_advance on a scratch session.
 *
 * DEFINITION.  Route of a slot under its current state, beam width B (1 <= B <= 8), T steps (1 <= T <= 16).  A hypothesis is (path,
 * total, state).  Start: one live hypothesis - empty path, total 0.0 (float64), the slot's state.  At step t, for every live hypothesis r:
 *   s(r, j)       exactly poi_score_rank's s(r, j): float(h_r) . items[j] in float32 from the same product routine, fragment loader and k
 *                 order; with wd non-NULL plus wd * sts[r][bin(last_poi[r], j)] for bin < n_dist.  A hypothesis with last_poi[r] < 0 (a fresh
 *                 slot at step 0) has no distance term.  A candidate's score is bit-equal to poi_score_rank's score_out for the same row
 *                 and POI.
 *   lse(r)        log sum_{j in [0, n_item)} exp(s(r, j)) over ALL POIs, excluded ones included: the model's distribution; exclusion only
 *                 limits what may be chosen.  float64: every float32 score is widened before exp; the result is max + log(float64 sum).
 *                 ORDER OF THE SUM - a function of the row's scores alone, not of the grid, the regime or the row's place in the call:
 *                 the POIs are cut into ITEM BLOCKS of 512 consecutive ids.  Inside a block, residue class l = j mod 32 (l = 0 .. 31) is
 *                 one chain in ascending j: a running maximum m and sum, sum = sum * exp(m - s) + 1 when s > m (m := s), else
 *                 sum += exp(s - m).  The 32 chains are rescaled to the block's maximum, sum_l * exp(m_l - M_b), and added by a
 *                 butterfly over l (partners l xor 16, 8, 4, 2, 1).  Over the blocks: M = the maximum of the M_b, then the terms
 *                 S_b * exp(M_b - M) are added in ASCENDING BLOCK ORDER, one serial chain from block 0; lse = M + log(S).  Scores are
 *                 expected finite (-inf is accepted and adds nothing).
 *   C(r)          [0, n_item) minus the slot's exclusion list minus the hypothesis's own path (the caller passes path_len = 0 to allow
 *                 revisits).
 *   NaN           a NaN score is never selected and adds nothing to the sum.
 *   expansion     r proposes its best min(B, |C(r)|) candidates by the tie rule of every top-K entry (higher score, then lower id), each
 *                 with total_r + (double(s) - lse(r)).
 *   merge         the slot keeps the best B of its at most B * B proposals: higher total, then lower parent beam index, then lower POI
 *                 id.  A survivor inherits its parent's state and path, appends the POI and is advanced by it.
 *   dead beams    fewer than B proposals leave dead beams: POI -1 from that step on, total -inf; they never come back and never propose.
 *                 A dead beam's parent_out is its own place (capped to n_par - 1), so that a gather stays in range.
 *
 * poi_route_expand - score + normaliser + top-b with exclusion, one pass over the item table for n hypothesis rows:
 *   users ... dd          poi_score_rank's arguments (users float32, items float32 or a registered half table, dim a multiple of 4 <= 256).
 *   path                  (n, path_stride) int32, path_len <= 16 valid ids per row (unsorted), or path_len = 0.
 *   ex_off, ex            exclusion lists in the conventions of poi_score_topk_near; row r uses list r / rows_per_list, so that the B rows of
 *                         a slot share one list (rows_per_list = 1: a list per row).  Both NULL = none.
 *   live                  (n) int32 or NULL: a row with live[r] == 0 is dead - it is not read and costs nothing.
 *   outputs               idx_out (n, b) by descending score, ties by ascending id, -1 where |C(r)| < b; score_out (n, b), -inf there;
 *                         lse_out (n) float64; count_out (n) or NULL = |C(r)|.
 *   bad rows              an exclusion list that is not ascending or leaves [0, n_item), or a path id outside [0, n_item): the row is
 *                         -1 / -inf / NaN lse / count 0 and is counted once (poi_ctx_take_bad_ids).  A dead row gives the same and is not counted.
 * No float atomics: identical calls give bitwise identical outputs, every grid and both regimes give the same outputs as every other, and
 * a row gives the same outputs alone as inside a larger call.  Two launch regimes: calls of at most "route_split_max" rows (a single
 * user's 1 .. 8 hypotheses is the live-traffic case) cut the item range of every 32-row tile over "route_grid" workgroups and finish the
 * rows in a second kernel; larger calls run one workgroup per 32-row tile, which finishes its own rows.  poi_ctx_last_plan: "route_path"
 * (0 tile, 1 split), "route_splits" (workgroups per tile, 0 on the tile path).  Timing name: "route_expand".  n = 0 is a no-op. */
int poi_route_expand(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                     const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                     int32_t n_dist, double dd,
                     const int32_t* path, int32_t path_stride, int32_t path_len, const int32_t* ex_off, const int32_t* ex, int32_t rows_per_list,
                     const int32_t* live, int32_t b,
                     int32_t* idx_out, float* score_out, double* lse_out, int32_t* count_out, void* stream);
/* The merge of one step: n_slot slots, n_par parent rows each (1 at step 0, B afterwards), b proposals per parent (n_par * b <= 64); idx /
 * score (n_slot * n_par, b) and lse (n_slot * n_par) are the expand outputs, total_in (n_slot, n_par) float64 the parents' totals, n_live
 * (n_slot) the number of live parents (a prefix of the slot's rows), NULL = all.  Outputs (n_slot, b) by the order above: parent_out,
 * poi_out (-1: dead), total_out (-inf: dead), steplp_out or NULL = double(score) - lse of the step (-inf: dead); nlive_out (n_slot) or NULL =
 * the live survivors.  Proposals with a -inf or NaN total sort last and come out dead.  One wavefront per slot, one proposal per lane.
 * Timing name: "route_merge". */
int poi_route_merge(poi_ctx* ctx, const int32_t* idx, const float* score, const double* lse, const double* total_in, const int32_t* n_live,
                    int32_t n_slot, int32_t n_par, int32_t b,
                    int32_t* parent_out, int32_t* poi_out, double* total_out, double* steplp_out, int32_t* nlive_out, void* stream);

/* ---- diversified recommendation (additive to 9): a fused pool of up to 64 candidates and its MMR re-ranking ------------------------------
 * Every other ranking entry answers "the K best POIs by score", and the K highest scores of an embedding model are routinely K
 * near-duplicates: the score is smooth in the item embedding and in the distance to the last check-in.  Re-ranking a candidate pool for
 * relevance against redundancy (maximal marginal relevance, MMR) is the serving step that fixes it.  Two stages, each an entry of its
 * own - the second also serves pools that come from elsewhere (poi_topk over explicit score rows) - and poi_diverse_topk, which runs both.
 *
 * Stage 1, the pool (poi_diverse_pool).
 *   C(r)          [0, n_item) minus ex[ex_off[r] .. ex_off[r + 1]): the conventions of poi_score_rank (ascending unique ids; both NULL = none).
 *   s(r, j)       exactly poi_score_rank's s(r, j): users[r] . items[j] in float32 from the same product routine and k order; with wd
 *                 non-NULL plus wd * sts[r][bin(last_poi[r], j)] for bin < n_dist (n_dist <= 4096).  A row with last_poi[r] < 0 has no
 *                 distance term.  wd NULL: the plain score; sts / thr / last_poi are then ignored.
 *   P(r)          the best m = min(pool, |selectable C(r)|) candidates by descending score, ties by ascending id.  NaN, -inf and +inf
 *                 scores are never pooled.  (+inf IS selected by poi_score_topk: a deviation, needed because stage 2 normalises the scores.)
 *   outputs       pool_idx (n, pool) int32 and pool_score (n, pool) float32, 1 <= pool <= 64, filled with -1 / -inf behind the m entries;
 *                 count_out (n) or NULL = |C(r)|.
 *   bad rows      as in poi_score_rank: a list that is not ascending or leaves [0, n_item) - the row is all -1 / -inf, count 0, counted
 *                 once (poi_ctx_take_bad_ids).
 *   items         float32 or a registered half table; rows >= n_item are never read.  dim: a multiple of 4, <= 256.  n = 0 is a no-op.
 * The walk of poi_score_rank / poi_group_topk: a workgroup owns a 32-row tile, the item tiles stream past on the f32 matrix pipe, every
 * wave keeps a sorted 64-entry list per row in LDS, exact to its last entry.  Two launch regimes: calls of at most "diverse_split_max"
 * rows (default 256) cut the item range into "diverse_grid" slices, a workgroup each, and merge the slices' lists in a second kernel;
 * larger calls run one workgroup per row tile.  poi_ctx_last_plan: "diverse_path" (0 tile, 1 split), "diverse_splits" (slices, 0 on the
 * tile path), "diverse_split_max" (the switch point in force).  Timing name: "diverse_pool".
 *
 * Stage 2, the re-rank (poi_diverse_rerank).  Per row a pool as above: position i is the i-th best, m = the entries before the first -1
 * (an id >= n_item among them rejects the row: all -1, counted once).  Everything below is float64.
 *   rel_i         (s_i - s_{m-1}) / (s_0 - s_{m-1}); every rel_i = 1 when s_0 == s_{m-1} (m == 1 included).
 *   d(i, l)       12742 * asin(min(1, sqrt(sin^2(dlat * pi/360) + cos(lat_i) cos(lat_l) sin^2(dlon * pi/360)))) km, cos(lat) from cphi.  This
 *                 is NOT the (1 - cos) / 2 form of cal_dis that the distance bins use: that form loses the relative accuracy of nearby
 *                 pairs to cancellation - harmless for the bins, whose thresholds are compared with the same term, but the similarity
 *                 is most sensitive exactly where POIs are metres apart.
 *   geo(i, l)     exp(-d(i, l) / scale_km), scale_km > 0.
 *   emb(i, l)     x_i . x_l / (|x_i| |x_l|), 0 if either norm is 0; x = the rows of items (float32 or a registered half table: the table
 *                 the score was taken with), dim a multiple of 4, <= 256.  One summation order per dim.
 *   sim           g * geo + (1 - g) * emb, g = geo_weight in [0, 1].  A part with zero weight is not evaluated: coords / cphi may be NULL
 *                 with g = 0, items with g = 1.
 *   selection     the first pick is position 0.  After the first pick l_0, pen_i = sim(i, l_0); after each further pick l,
 *                 pen_i = max(pen_i, sim(i, l)).  Step t >= 1 picks the unselected i with the largest
 *                 obj_i = trade * rel_i - (1 - trade) * pen_i, ties to the lower position; min(k, m) picks.  trade in [0, 1]; trade = 1
 *                 returns the pool's first k entries unchanged (and evaluates no similarity).
 *   outputs       idx_out (n, k) the POI ids, -1 fill, 1 <= k <= 32, k <= pool <= 64; score_out (n, k) or NULL: the ORIGINAL float32
 *                 scores, -inf fill; pos_out (n, k) or NULL: the pool positions, -1 fill; obj_out (n, k) float64 or NULL: the objective
 *                 at selection (trade * rel_0 for the first pick), -inf fill.
 * One wavefront per row, one pool position per lane.  No atomics touch a result: a row's bits do not depend on the grid, on its place
 * in the call or on the other rows.  Timing name: "diverse_rerank".  n = 0 is a no-op.
 *
 * poi_diverse_topk runs both: the arguments are the union of the two, coords / cphi serve the distance term and the geo part alike,
 * items the score and the embedding part.  pool_idx / pool_score (both or neither) receive the pool; NULL keeps it in a context-owned
 * workspace.  No host synchronisation between the stages.  Its output equals the two calls' bit for bit. */
int poi_diverse_pool(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                     const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                     int32_t n_dist, double dd,
                     const int32_t* ex_off, const int32_t* ex, int32_t pool,
                     int32_t* pool_idx, float* pool_score, int32_t* count_out, void* stream);
int poi_diverse_rerank(poi_ctx* ctx, const int32_t* pool_idx, const float* pool_score, int32_t n, int32_t pool,
                       const float* items, int32_t n_item, int32_t dim, const double* coords, const double* cphi,
                       int32_t k, double trade, double geo_weight, double scale_km,
                       int32_t* idx_out, float* score_out, int32_t* pos_out, double* obj_out, void* stream);
int poi_diverse_topk(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                     const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                     int32_t n_dist, double dd,
                     const int32_t* ex_off, const int32_t* ex, int32_t pool,
                     int32_t k, double trade, double geo_weight, double scale_km,
                     int32_t* idx_out, float* score_out, int32_t* pos_out, double* obj_out,
                     int32_t* pool_idx, float* pool_score, int32_t* count_out, void* stream);

/* ---- candidate generation (additive to 9): the exact top-K of every row for K up to 4096 ---------------------------------------------------
 * Every other ranking entry stops at a short list (k <= 32 fused, k <= 64 in poi_topk): each keeps a sorted list with one entry per
 * lane of a wavefront.  The retrieval stage of a two-stage recommender hands hundreds to thousands of candidates per user to a
 * downstream ranker, and "recall of the retrieval stage at K" is the number such a system is tuned on.  These entries SELECT (radix
 * selection over explicit score rows) instead of inserting into a sorted list.
 *   C(r)          [0, n_item) minus ex[ex_off[r] .. ex_off[r + 1]): the conventions of poi_score_rank / poi_score_topk_near (ascending
 *                 unique ids; both NULL = none).
 *   selectable    an entry of C(r) is selectable unless its score is NaN or -inf.  +inf IS selectable, as in poi_score_topk.
 *   order         the result of row r is the best K' = min(k, |selectable|) entries under the tie rule of every top-K entry: higher
 *                 score first, then the lower id.  idx_out (n, k) is sorted best first, -1 ids and -inf scores (score_out (n, k) or
 *                 NULL) behind the K' entries.
 *   count_out     (n) or NULL: |C(r)|, not clipped to k and not reduced by the scores that are not selectable.
 *   limits        1 <= k <= min(4096, n_item), otherwise POI_ENOTSUP.
 *   signed zeros  -0.0 and +0.0 are the SAME score and the id decides - poi_score_rank compares with float > / ==, and the two entries
 *                 agree on every row.  A selected zero is written to score_out as +0.0 whichever sign it had.  (poi_topk leaves the
 *                 order of -0.0 against +0.0 unspecified.)
 *   bad rows      the rule of poi_score_rank: a row whose list is not ascending or leaves [0, n_item) is rejected - all -1 / -inf,
 *                 count 0, counted once (poi_ctx_take_bad_ids).
 *   determinism   the selected set follows from integer counts and the order from a total order: identical bits on every grid, in
 *                 both launch regimes, for any chunking, and for a row alone or in a call of thousands.  No float atomics.
 *
 * poi_score_rows writes s(r, j) of poi_score_rank for every pair into scores_out[r * ld + j] (ld >= n_item; the columns beyond n_item
 * are not written): users[r] . items[j] from the same product routine and k order, with wd non-NULL plus wd * sts[r][bin(last_poi[r], j)]
 * for bin < n_dist by the same expression; a row with last_poi[r] < 0 has no distance term.  The bits are poi_score_rank's score_out.
 * users .. dd are poi_score_rank's arguments (items float32 or a registered half table; dim a multiple of 4, <= 256).  A store-epilogue
 * instance of poi_score_rank's tile walk: unlike poi_score_all it needs no (n, n_item) probability matrix for the distance term.
 * Timing name: "score_rows".  n = 0 is a no-op.
 *
 * poi_topk_select is the definition above on explicit float32 score rows scores (n, ld), the first n_item columns of a row being its
 * scores: the large-K counterpart of poi_topk for the models whose score is not users . items, and an independent check of the
 * selection.  Three digit passes (11 / 11 / 10 bits of the order-preserving integer image of the score) count the entries that share
 * the prefix found so far - per (row, slice) in LDS, summed per row with integer atomic adds - and fix the exact K'-th key; everything
 * above it is collected in any order, of the entries equal to it exactly the lowest ids; one workgroup per row sorts the K' entries.
 * Two launch regimes: calls of at most "select_split_max" rows (poi_ctx_set_option, default 256) cut each row's id range into
 * "select_grid" slices (0: by the row count and the CUs; at most 64), a workgroup each; larger calls run one workgroup per row.
 * poi_ctx_last_plan: "select_path" (0 row, 1 split), "select_splits" (slices, 0 on the row path).  Timing name: "topk_select" (its
 * stages: "select_pass0" / "select_pass1" / "select_pass2" / "select_collect" / "select_sort").  n = 0 is a no-op.
 *
 * poi_score_candidates runs both with the score rows in a context-owned workspace: a whole number of 32-row tiles at a time, as many
 * as fit "select_chunk_mb" MiB (default 1024; at least one tile), no host synchronisation between the chunks.  Its output equals
 * poi_score_rows + poi_topk_select bit for bit, whatever the chunk.  poi_ctx_last_plan: "select_rows_per_chunk", "select_chunks",
 * "select_path", "select_splits".  Timing name: "score_candidates" (around "score_rows" and "topk_select" of every chunk). */
int poi_score_rows(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                   const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                   int32_t n_dist, double dd,
                   float* scores_out, int64_t ld, void* stream);
int poi_topk_select(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, int64_t ld, int32_t k,
                    const int32_t* ex_off, const int32_t* ex,
                    int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);
int poi_score_candidates(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                         const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                         int32_t n_dist, double dd,
                         int32_t k, const int32_t* ex_off, const int32_t* ex,
                         int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- re-ranking (additive to 9): score explicit candidate lists, blend with a prior, exact top-K ---------------------------------------------
 * The second stage of a two-stage recommender: a cheap model (or a campaign, a geofence, "open now") has produced candidate POIs per
 * row - e.g. the idx_out of poi_score_candidates - and THIS model scores exactly those and returns them in order.  No (n, n_item) matrix.
 *   lists         ragged (cand_off non-NULL): row r owns cand[cand_off[r] .. cand_off[r + 1]), cand holds n_cand ids in all; scores
 *                 and priors are flat and parallel to cand.  Shared (cand_off NULL): ONE list cand[0 .. n_cand) for every row; scores
 *                 and priors are (n, n_cand) row-major.
 *   ids           an id in [0, n_item) is scored; duplicates are allowed and get identical bits.  A NEGATIVE id is padding: its score
 *                 is -inf and it is never selected - the (n, k) idx_out of poi_score_candidates with its -1 fill is a ragged list with
 *                 cand_off[r] = r k.
 *   score         s(r, j) of poi_score_rows / poi_score_rank, bit for bit: users[r] . items[j] from the same product routine and k
 *                 order, with wd non-NULL plus wd * sts[r][bin(last_poi[r], j)] for rows with last_poi[r] >= 0.  users .. dd are
 *                 poi_score_rank's arguments (items float32 or a registered half table; dim a multiple of 4, <= 256).
 *   bad rows      a ragged row whose offsets are negative, descending or end beyond n_cand, or that holds an id >= n_item, is
 *                 rejected: the entries it owns (where its offsets say so at all) are -inf, it is counted once
 *                 (poi_ctx_take_bad_ids), and nothing outside cand[0 .. n_cand) or the tables is read.  A shared list that holds an
 *                 id >= n_item rejects every row of the call, counted once.  Entries of cand that no accepted row owns get -inf.
 *
 * poi_score_lists writes the scores: score_out (n_cand) ragged, (n, n_cand) shared.  Ragged lists go through one workgroup per (row,
 * chunk of poi_score_lists_chunk() entries) - the row's fragment against 32 gathered item rows per product, one item row of
 * 4 dim bytes per entry; a shared list through a real 32 x 32 tile product, each item row fetched once per 32-row tile.  An output
 * element depends on its own (row, id) only: every grid gives the same bits.  poi_ctx_last_plan: "lists_path" (0 ragged, 1 shared).
 * Timing name: "score_lists".  n = 0 or n_cand = 0 is a no-op.
 *
 * poi_rerank_lists orders every list under EXPLICIT scores.  The key of entry i of row r is
 *   t = score[i]                                                          prior == NULL (the weights are ignored)
 *   t = (float)(w_score * (double)score[i] + w_prior * (double)prior[i])  otherwise; both products and the sum are rounded to double
 *                                                                          one by one (no contraction), the result once to float
 * An entry is selectable unless its id is negative or t is NaN or -inf (+inf is selectable; -0.0 and +0.0 are ONE key, written as +0.0:
 * the rules of poi_score_candidates).  Total order: higher t, then the lower id, then the lower position in the list; duplicates are
 * kept.  Outputs for 1 <= k <= 4096, the best K' = min(k, selectable) entries sorted best first: idx_out (n, k), -1 beyond K';
 * score_out (n, k) or NULL: the key t, -inf beyond K'; pos_out (n, k) or NULL: the entry's position inside its row's list (-1 beyond
 * K') - what a caller gathers side data with, and how far an entry moved; count_out (n) or NULL: the number of selectable entries, not
 * clipped to k.  One workgroup per row, a bitonic network over the next power of two in LDS; integer and compare work only: the same
 * bits for a row alone or in a call of thousands.  A ragged row with malformed offsets or more than 4096 entries is rejected (all
 * -1 / -inf, count 0, counted once); ids are not checked against a table here.  A shared n_cand > 4096 or k outside [1, 4096] is
 * POI_ENOTSUP.  Timing name: "rerank_lists".  n = 0 is a no-op.
 *
 * poi_rerank runs both with the scores in a context-owned workspace, no host synchronisation in between; its output equals
 * poi_score_lists + poi_rerank_lists bit for bit, and a row either stage rejects is counted once.  Timing name: "rerank" (around
 * "score_lists" and "rerank_lists"). */
int poi_score_lists_chunk(void);      /* entries of a ragged row per workgroup step (a compile-time constant; tests straddle it) */
int poi_score_lists(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                    const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                    int32_t n_dist, double dd,
                    const int32_t* cand_off, const int32_t* cand, int32_t n_cand, float* score_out, void* stream);
int poi_rerank_lists(poi_ctx* ctx, const int32_t* cand_off, const int32_t* cand, int32_t n, int32_t n_cand,
                     const float* score, const float* prior, double w_score, double w_prior, int32_t k,
                     int32_t* idx_out, float* score_out, int32_t* pos_out, int32_t* count_out, void* stream);
int poi_rerank(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
               const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
               int32_t n_dist, double dd,
               const int32_t* cand_off, const int32_t* cand, int32_t n_cand, const float* prior, double w_score, double w_prior, int32_t k,
               int32_t* idx_out, float* score_out, int32_t* pos_out, int32_t* count_out, void* stream);

/* ---- filtered recommendation (additive to 9): the top-K among the POIs that pass an attribute predicate -----------------------------------
 * "The best restaurants for this user", "the best museums open now", "the best cafes within 2 km": a top-K over the POIs that pass a
 * predicate on the CALLER'S attributes (the reference data carries ids, times and coordinates only).  Passing the complement as an
 * exclusion list costs a binary search per id over a list as long as the table; these entries take a pass BITMAP instead.
 *
 * Attributes, per POI, both optional:  cat (n_item) int32 in [0, n_cat), 1 <= n_cat <= 4096;  flags (n_item) uint32, whose meaning is
 * the application's (price tier, open now, ...).  A NULL flags reads as all-zero words.
 * Predicate q of a table of P:  a category list pc[pc_off[q] .. pc_off[q + 1]) (ids ascending and unique; EMPTY = any category) and
 * three words need[q] / any[q] / forbid[q]:
 *   pass(q, j) = (list empty or cat[j] in list) and (flags[j] & need) == need and (any == 0 or (flags[j] & any) != 0)
 *                and (flags[j] & forbid) == 0
 * A NULL cat (or pc) with a non-empty list is POI_EINVAL.  A POI whose cat[j] lies outside [0, n_cat) passes no predicate that has a
 * list and is counted once per POI (poi_ctx_take_bad_ids).
 *
 * poi_filter_build writes bits_out (P, ldw) uint32, ldw >= W = ceil(n_item / 32): POI j is bit j & 31 of word j >> 5 of its
 * predicate's row; the bits at j >= n_item (the pad words included) are written as 0.  count_out (P) int32 or NULL: the popcounts.
 * All arrays are device memory.  One small kernel, integer work only; the predicate words are copied aside before it runs, so
 * bits_out may overlap them.  Timing name: "filter_build".  P = 0 is a no-op.  The ranking
 * entries take ONLY the bitmap: a caller with a predicate of its own (opening hours evaluated at query time) packs a mask itself.
 *
 * The ranking entries:
 *   C(r)          { j in [0, n_item) : bit j of row pred[r] of bits
 *                   and (anchor[r] < 0 or c_r == +inf or c(anchor[r], j) < c_r or j == anchor[r])
 *                   and j not in ex[ex_off[r] .. ex_off[r + 1]) }
 *                 c, c_r, anchor and lat_order as poi_score_topk_near - with ONE difference: the anchor is a candidate only if it
 *                 passes the predicate too.  pred (n) int32, or NULL: every row uses predicate 0.  bits is (n_pred, ldw); its bits
 *                 at j >= n_item are ignored, never trusted.
 *   score         poi_score_rank's s(r, j), BIT FOR BIT, on every path: users[r] . items[j] from the same product routine and k
 *                 order; with wd non-NULL plus wd * sts[r][bin(anchor[r], j)] for bin < n_dist by the same expression (the anchor
 *                 doubles as last_poi; a row with anchor[r] < 0 has no distance term).  poi_score_topk_near sums in another order,
 *                 which is why it was not extended.  One score definition: the path taken changes no bit of the result.
 *   order, fill, selectable, signed zeros, determinism: as poi_score_candidates - higher score first, then the lower id; -1 ids and
 *                 -inf scores behind the K' = min(k, |selectable|) entries; NaN and -inf are not selectable, +inf is; -0.0 and +0.0
 *                 are one score, written as +0.0; identical bits on every grid, in both regimes, alone or in a call of thousands.
 *   count_out     (n) or NULL: |C(r)|, not clipped to k and not reduced by the scores that are not selectable.
 *   bad rows      pred[r] outside [0, n_pred), an anchor outside [-1, n_item), an exclusion list that is not ascending or leaves
 *                 [0, n_item): all -1 / -inf, count 0, counted once (poi_ctx_take_bad_ids).
 *   limits        1 <= k <= 32; dim a multiple of 4, <= 256; items float32 or a registered half table; n_dist <= 4096 with the
 *                 distance term.  Otherwise POI_ENOTSUP.  No float atomics on any result.
 *
 * poi_score_topk_filtered - users .. dd are poi_score_rank's arguments with anchor in last_poi's place.  path:
 *   POI_FILTER_WALK    the tile walk of poi_diverse_pool with lists of k <= 32.  A 32-item tile is one bitmap word per row; a tile
 *                      whose 32 words are all zero costs neither a product nor an item-row load, so the walk scales with the
 *                      selectivity when the rows of a tile share a predicate.  A finite radius is POI_ENOTSUP here.
 *   POI_FILTER_GATHER  one workgroup per row and slice: the set bits (without a radius) or the latitude band (with one: the exact
 *                      Haversine test, then the bit) are compacted into a queue, and the queue is scored by the walk's product
 *                      routine on gathered item rows.  Cost per CANDIDATE, not per POI.
 *   POI_FILTER_AUTO    gather when c_r is finite, or when cand_hint > 0 and n * cand_hint * G < ceil(n / 32) * n_item; otherwise
 *                      walk.  cand_hint: the caller's upper bound on the pass count of the predicates the call uses, 0 = unknown.
 *                      G: option "filter_gather_cost" (DESIGN.md section 27 has the table it is read from).
 * Calls of at most "filter_split_max" rows (default 256) cut the item range / every row's candidates into "filter_grid" slices (0: by
 * the row count and the CUs; at most 64), a workgroup each, and merge.  poi_ctx_last_plan: "filter_path" (1 walk, 2 gather),
 * "filter_splits" (0 outside the split regime), "filter_split_max".  Timing name: "score_topk_filtered".  n = 0 is a no-op.
 *
 * poi_topk_filtered_scores is the definition (without a radius) on explicit float32 score rows scores (n, ld), ld >= n_item, one
 * workgroup per row: the counterpart of poi_topk / poi_rank_scores for the models whose score is not users . items, and an independent
 * check of the fused paths.  Timing name: "topk_filtered_scores".  n = 0 is a no-op. */
enum { POI_FILTER_AUTO = 0, POI_FILTER_WALK = 1, POI_FILTER_GATHER = 2 };
int poi_filter_build(poi_ctx* ctx, const int32_t* cat, const uint32_t* flags, int32_t n_item, int32_t n_cat,
                     const int32_t* pc_off, const int32_t* pc, const uint32_t* need, const uint32_t* any, const uint32_t* forbid, int32_t P,
                     uint32_t* bits_out, int64_t ldw, int32_t* count_out, void* stream);
int poi_score_topk_filtered(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                            const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor,
                            int32_t n_dist, double dd,
                            const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred, int64_t cand_hint,
                            const int32_t* lat_order, double c_r, const int32_t* ex_off, const int32_t* ex, int32_t k, int32_t path,
                            int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);
int poi_topk_filtered_scores(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, int64_t ld,
                             const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred,
                             const int32_t* ex_off, const int32_t* ex, int32_t k,
                             int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);

/* ---- capped recommendation (additive to 9): the top-K with at most `per` POIs of one label -------------------------------------------------
 * "The best 20 places, but no more than 2 of the same category" (or chain, or neighbourhood) - the hard cap of a carousel; with a cap of
 * 1, "which kinds of place for this user, and the best one of each".  poi_diverse_topk trades relevance against similarity softly
 * inside a pool of 64 and can promise no cap; poi_score_topk_filtered restricts to one predicate and does not spread over labels.
 *
 *   labels        (n_item) int32, device.  labels[j] >= 0 names POI j's group; labels[j] < 0 means unlabelled: the POI is a group of
 *                 its own and is never capped.  The ranking entries index nothing by a label: any non-negative value is a group.
 *   cap           1 <= per <= 32, and 1 <= k <= 32.
 *   C(r)          poi_score_topk_filtered's candidate set without a radius: bit j of row pred[r] of bits (bits == NULL: every POI
 *                 passes, and ldw / n_pred / pred are ignored) minus ex[ex_off[r] .. ex_off[r + 1]).
 *   score         poi_score_rank's s(r, j), BIT FOR BIT: users[r] . items[j] from the same product routine and k order, plus - with
 *                 wd non-NULL - wd * sts[r][bin(anchor[r], j)] for bin < n_dist (the anchor in last_poi's place; a row with
 *                 anchor[r] < 0 has no distance term), exactly as poi_score_topk_filtered has it.
 *   order, zeros  higher score first, then the lower id; -0.0 and +0.0 are one score, written as +0.0; NaN and -inf are not
 *                 selectable, +inf is.
 *   result        walk the selectable members of C(r) in that order; take j unless labels[j] >= 0 and `per` entries already taken
 *                 carry labels[j]; stop at k.  Equivalently: j is kept iff fewer than `per` selectable candidates of its label
 *                 precede it, and the list is the first k kept.  -1 ids and -inf scores behind them, as poi_score_candidates.
 *   outputs       idx_out (n, k); score_out (n, k) or NULL; label_out (n, k) or NULL: labels[idx], -1 on the fill; count_out (n) or
 *                 NULL: |C(r)|, neither clipped to k nor reduced by the cap.
 *   bad rows      as poi_score_topk_filtered: pred[r] outside [0, n_pred), an anchor outside [-1, n_item), an exclusion list that is
 *                 not ascending or leaves [0, n_item): all -1 / -inf, count 0, counted once (poi_ctx_take_bad_ids).
 *   limits        dim a multiple of 4, <= 256; items float32 or a registered half table; n_dist <= 4096 with the distance term; no
 *                 radius.  k, per or dim outside their range: POI_ENOTSUP.  NULL labels: POI_EINVAL.  n = 0 is a no-op.
 *   determinism   no float atomics; identical bits on every grid, in both launch regimes, for a row alone or in a call of thousands.
 * It follows that the list for k' < k is a prefix of the list for k; that with per >= k, with all labels distinct or with all labels
 * negative the result is poi_score_topk_filtered's / poi_topk_filtered_scores' bit for bit; and that with one label for every POI the
 * list is the plain top-`per`.
 *
 * The fill gate.  The kernels skip a candidate that does not beat entry g - 1 of its row's list.  Under a cap the list may never reach
 * k entries (five labels with per = 2 fill 10), so g = min(k, fill[pred[r]][per]) with fill (max(n_pred, 1), 33) int32 from
 * poi_labels_build:  fill[q][m] = #(unlabelled POIs passing q) + sum over the labels of min(m, #POIs of the label passing q),  the
 * longest list predicate q can give under the cap m.  fill == NULL means g = k: correct, but every (row, POI) pair of a row whose list
 * cannot fill takes the serial path.  Any value at or above the true one is safe, only slower; a value BELOW it is a caller error that
 * yields lists cut at that value.  Exclusion lists are not in fill: a row whose list empties a label stays correct and slow.
 *
 * poi_labels_build - labels, and bits (n_pred, ldw) or NULL with n_pred = 0 (one row: every POI passes).  Requires
 * 1 <= n_label <= n_item.  Writes fill_out (max(n_pred, 1), 33) and, if not NULL, count_out (n_label): the POIs of every label in
 * [0, n_label), whatever they pass.  A label >= n_label is counted once per POI (poi_ctx_take_bad_ids) and entered as unlabelled, which
 * keeps fill an upper bound.  Integer atomics on a context-owned histogram only, at most "capped_hist_kb" KiB of it at a time.
 * Timing name: "labels_build" (once per chunk of predicates).
 *
 * poi_score_topk_capped - the counterpart of poi_score_topk_filtered(path = POI_FILTER_WALK): users .. dd are poi_score_rank's
 * arguments with anchor in last_poi's place; the same tile walk with 32-entry lists that carry the label of every entry, a cap-aware
 * insertion, and pairwise merges of the waves' and the slices' lists with the cap re-applied after each (DESIGN.md section 30 says why
 * a plain best-64 followed by one cap is wrong).  Calls of at most "capped_split_max" rows (default 256) cut the item range of every
 * 32-row tile into "capped_grid" slices (0: by the row count and the CUs; at most 64), a workgroup each, and merge.
 * poi_ctx_last_plan: "capped_splits" (0 outside the split regime), "capped_split_max".  Timing name: "score_topk_capped", with
 * "capped_walk" and "capped_merge" inside it.
 *
 * poi_topk_capped_scores - the counterpart of poi_topk_filtered_scores: the definition on explicit float32 score rows scores (n, ld),
 * ld >= n_item, one workgroup per row, for the models whose score is not users . items, and an independent check of the walk.  Timing
 * name: "topk_capped_scores". */
int poi_labels_build(poi_ctx* ctx, const int32_t* labels, int32_t n_item, int32_t n_label,
                     const uint32_t* bits, int64_t ldw, int32_t n_pred, int32_t* count_out, int32_t* fill_out, void* stream);
int poi_score_topk_capped(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                          const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor,
                          int32_t n_dist, double dd,
                          const int32_t* labels, int32_t per, const int32_t* fill,
                          const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred,
                          const int32_t* ex_off, const int32_t* ex, int32_t k,
                          int32_t* idx_out, float* score_out, int32_t* label_out, int32_t* count_out, void* stream);
int poi_topk_capped_scores(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, int64_t ld,
                           const int32_t* labels, int32_t per, const int32_t* fill,
                           const uint32_t* bits, int64_t ldw, int32_t n_pred, const int32_t* pred,
                           const int32_t* ex_off, const int32_t* ex, int32_t k,
                           int32_t* idx_out, float* score_out, int32_t* label_out, int32_t* count_out, void* stream);

/* ---- label recommendation (additive to 9): which category / district comes next, by probability mass ---------------------------------------
 * The level above the POI lists: the probability that the next check-in falls in label l is the softmax mass of the label's POIs,
 *   p(l | r) = sum over j in l of exp(s(r, j)) / sum over j of exp(s(r, j)),
 * computed in one fused pass without the (n, n_item) score matrix.  poi_score_topk_capped(per = 1) ranks labels by their single best POI;
 * a label with 400 decent POIs can outweigh one with a single excellent POI, and only the mass says so.
 *
 *   rows, s(r, j)  exactly poi_score_rank's: the same product routine, fragment loader and k order, the same distance term at the row's
 *                  `anchor` (no term while anchor < 0), one zero; float32 and half item tables
 *   labels         (n_item) int32, a PoiLabels' device array: a value in [0, n_label) is POI j's label, anything else (< 0) is unlabelled
 *                  and goes to the extra bucket n_label.  1 <= n_label <= n_item
 *   C(r)           every POI minus the row's exclusion list (ex_off (n + 1), ex: CSR, ascending ids, both NULL = none; the checks of
 *                  poi_score_topk_capped).  A NaN or -inf score is no candidate and adds nothing
 *   M(r)           the maximum of s(r, j) over ALL j in [0, n_item) with a non-NaN score: it does not depend on the exclusion list
 *   q(r, j)        round_to_nearest_uint64(exp(double(s(r, j)) - double(M(r))) * 2^36), per candidate
 *   per bucket     mass_q = the uint64 sum of q over the bucket's candidates; best = the candidate that wins under the top-K tie rule
 *                  (higher score, then lower id); count = its candidates.  An integer sum, a maximum under a total order, an integer
 *                  count: their bits do not depend on the grid, the regime, the accumulator's home, the chunking of the rows or on whether
 *                  a row is served alone or with thousands of others.  n_item < 2^27 keeps the sum below 2^63 (larger: POI_ENOTSUP)
 *   resolution     one q unit is 2^-36 of the row's best POI: rounding each term to it leaves an ABSOLUTE ERROR FLOOR of 2^-37 of the best
 *                  POI's weight per candidate of a label's mass (a candidate more than 25.6 below M(r) adds nothing)
 *   total_q        the sum over all n_label + 1 buckets;  logp(r, l) = log(double(mass_q)) - log(double(total_q)) in float64, -inf for a
 *                  label without mass;  the log-normaliser over the candidates is lognorm = M + log(total_q * 2^-36), -inf without mass
 *   fill           a row with non-finite M(r) (no scorable POI, all NaN, a +inf score) has no candidates: masses and counts 0, ids -1,
 *                  scores and log values -inf.  A rejected row (anchor outside [-1, n_item), malformed exclusion list) is counted once
 *                  in the context's bad-id counter, comes out the same way and reports M = -inf
 *
 * poi_score_labels - the dense result for n rows: mass_out (n, n_label + 1) uint64, best_id_out / best_score_out / count_out of the
 * same shape (id -1 and score -inf for an empty bucket), m_out (n) float32, lognorm_out (n) float64; every output may be NULL and is
 * then skipped.  The category distribution as a feature for a downstream ranker.
 *
 * poi_score_topk_labels - the best k labels (1 <= k <= 32, otherwise POI_ENOTSUP) per row among the labels with count > 0; the
 * unlabelled bucket is never listed, its share is rest_logp_out (n).  by = POI_LABELS_BY_MASS: higher mass_q first, then the lower
 * label id; POI_LABELS_BY_MAX: by the label's best POI under the top-K tie rule - the labels, ids and scores of
 * poi_score_topk_capped(per = 1) on labellings without unlabelled POIs.  label_out (n, k) int32 (-1 fill), logp_out (n, k) float64
 * (-inf fill), best_id_out / best_score_out (n, k) the listed labels' best POIs; n_listed_out, rest_logp_out, m_out, lognorm_out (n).
 * All but label_out may be NULL.
 *
 * poi_labels_scores - the same definition on explicit float32 score rows scores (n, ld), ld >= n_item, one workgroup per row, for the
 * models whose score is not users . items, and an independent check of the walk: the dense outputs, and with 1 <= k <= 32 the top-K
 * outputs (k = 0: none).
 *
 * Kernels (labels.hip): a max-only instance of the tile walk gives M(r) ("labels_max"), a second walk accumulates ("labels_walk") with
 * integer atomics only - in the workgroup's LDS while the accumulators fit "labels_lds_kb", else on the context's global accumulator -
 * and a finish kernel ("labels_finish") takes logs and selects the k labels.  Few rows cut every tile's item range into slices
 * ("labels_split_max" / "labels_grid").  poi_ctx_last_plan: "labels_splits" (0 outside the split regime), "labels_split_max",
 * "labels_home" (1 LDS, 2 global), "labels_chunks", "labels_rows_per_chunk". */
#define POI_LABELS_BY_MASS 0
#define POI_LABELS_BY_MAX 1
int poi_score_labels(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                     const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor,
                     int32_t n_dist, double dd,
                     const int32_t* labels, int32_t n_label, const int32_t* ex_off, const int32_t* ex,
                     uint64_t* mass_out, int32_t* best_id_out, float* best_score_out, int32_t* count_out, float* m_out, double* lognorm_out,
                     void* stream);
int poi_score_topk_labels(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                          const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* anchor,
                          int32_t n_dist, double dd,
                          const int32_t* labels, int32_t n_label, const int32_t* ex_off, const int32_t* ex, int32_t by, int32_t k,
                          int32_t* label_out, double* logp_out, int32_t* best_id_out, float* best_score_out, int32_t* n_listed_out,
                          double* rest_logp_out, float* m_out, double* lognorm_out, void* stream);
int poi_labels_scores(poi_ctx* ctx, const float* scores, int32_t n, int32_t n_item, int64_t ld,
                      const int32_t* labels, int32_t n_label, const int32_t* ex_off, const int32_t* ex, int32_t by, int32_t k,
                      uint64_t* mass_out, int32_t* best_id_out, float* best_score_out, int32_t* count_out,
                      int32_t* label_out, double* logp_out, int32_t* top_id_out, float* top_score_out, int32_t* n_listed_out,
                      double* rest_logp_out, float* m_out, double* lognorm_out, void* stream);

/* ---- audience recommendation (additive to 9): given a POI, which users? -------------------------------------------------------------------
 * Every entry above ranks POIs for a row.  poi_score_audience ranks ROWS for a POI: for query POIs pois[q] (q < n_q) and the candidate
 * rows users (n, dim) it returns per query the best rows under the score and the order of poi_score_rank / poi_score_rows:
 *   s(u, j)  = users[u] . items[j] (+ wd * sts[u][bin(last_poi[u], j)] with wd non-NULL, for a row with last_poi[u] >= 0), to the bit;
 *   C(q)     = [0, n) minus ex[ex_off[q] .. ex_off[q + 1]) - ascending unique ROW INDICES, typically the rows that already visited the
 *              POI; both pointers NULL: no exclusion;
 *   result   = the best min(k, |C(q)|) rows of C(q) by descending score, ties by ascending row index, into idx_out / score_out (n_q, k);
 *              -1 ids and -inf scores behind them; count_out[q] = |C(q)|, not clipped to k.  A NaN score is never listed.
 * The first 13 arguments are poi_score_rank's: items float32 or a registered half table, dim a multiple of 4 up to 256, sts
 * (n, n_dist + 1), last_poi (n); n_dist at most 1024 with the distance term.  1 <= k <= 32 (POI_ENOTSUP beyond: poi_audience_rows +
 * poi_topk_select is the route for a larger k).  A query id outside [0, n_item), or a list that is not ascending or leaves [0, n), rejects the
 * query: -1 / -inf, count 0, counted once (poi_ctx_take_bad_ids) - poi_score_rank's rule.  The same POI may be queried twice: two
 * identical rows.  n_q = 0 is a no-op; n = 0 with n_q > 0 writes the empty lists.
 * A workgroup keeps a block of 32 query POIs resident and streams the user table past them: per query block the user table is read
 * once.  Two launch regimes: calls of at most "audience_split_max" queries (poi_ctx_set_option, default 256: live traffic, a few POIs
 * against every user) cut the rows into "audience_grid" slices, one workgroup per (query block, slice), and merge the slices' lists in
 * a second kernel; larger calls run one workgroup per query block.  The output is bitwise the same on every grid and in both regimes,
 * for a query alone or among thousands, wherever it stands in its block; no float atomics.  poi_ctx_last_plan: "audience_path",
 * "audience_splits", "audience_split_max".  Timing names: "score_audience" (the call), and inside it "audience_walk" and - split regime -
 * "audience_merge".
 *
 * poi_audience_rows is the same walk with a store epilogue: scores_out[q * ld + u] = s(u, pois[q]) for u < n (ld >= n; the columns beyond
 * n are not written); the row of a rejected query (id outside [0, n_item)) is -inf.  The large-k route (with poi_topk_select: there n is
 * n_q and n_item the candidate count) and an independent check of poi_score_audience.  Timing name: "audience_rows". */
int poi_score_audience(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                       const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                       int32_t n_dist, double dd,
                       const int32_t* pois, int32_t n_q, const int32_t* ex_off, const int32_t* ex, int32_t k,
                       int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);
int poi_audience_rows(poi_ctx* ctx, const float* users, const float* items, int32_t n, int32_t n_item, int32_t dim,
                      const float* wd, const float* sts, const double* coords, const double* cphi, const double* thr, const int32_t* last_poi,
                      int32_t n_dist, double dd,
                      const int32_t* pois, int32_t n_q, float* scores_out, int64_t ld, void* stream);

/* ---- similar POIs and users (additive to 9): places like this one, users like this one, "because you visited X" ------------------------------
 * Every entry above starts from a user row or ranks rows for a POI.  These rank the rows of ONE table x (n, dim) - the POI table, or a
 * table of user rows - by their similarity to a query row of the same table, without an (n, n) matrix and without a normalised copy of
 * the table.  dim a multiple of 4 up to 256; x float32 or a registered half table.
 *   inv[i]    = 1 / sqrt(sum_c x[i][c]^2) in float64, 0 for a zero row.  Summation order: poi_diverse_rerank's - four interleaved fma
 *               chains over the float4 columns (chain q takes the columns 4 i + q), closed as (a0 + a1) + (a2 + a3): one order per dim.
 *   emb(i, j) = (double)dot32(i, j) * (inv[i] * inv[j]);  dot32 = the float32 product of poi_score_rows for row x[i] against item x[j],
 *               to the bit.  Not clamped; 0 for a zero row.
 *   geo(i, j) = exp(-d(i, j) / scale_km), d = poi_diverse_rerank's sin^2 Haversine distance (km), operation for operation, in float64,
 *               cos(lat) from cphi.
 *   sim(i, j) = (float)(g geo + (1 - g) emb), g = geo_weight in [0, 1) (g = 1 is POI_EINVAL), scale_km > 0: formed in float64 without
 *               contraction, rounded once to float32; -0.0 is written as +0.0.  With g = 0 nothing of geo is evaluated and coords / cphi
 *               may be NULL.  sim(i, j) and sim(j, i) are the same bits.
 *   C(q)      = [0, n) minus the query's own row queries[q], minus ex[ex_off[q] .. ex_off[q + 1]) (ascending unique row indices; both
 *               NULL: none).  A list that names the query row itself does not subtract it twice.
 *   result    = the best min(k, |C(q)|) rows of C(q) by descending sim, ties by ascending row, into idx_out / score_out (n_q, k); -1 ids
 *               and -inf scores behind them; count_out[q] = |C(q)|, not clipped to k.  A NaN is never listed.
 * A query outside [0, n), or a list that is not ascending or leaves [0, n), rejects the query: -1 / -inf, count 0, counted once
 * (poi_ctx_take_bad_ids) - poi_score_audience's rule.  The same row may be queried twice.  n_q = 0 is a no-op; n > 0.
 * This is a similarity of the model's rows, nothing more: it is not a decomposition of any model score.
 *
 * poi_row_inv_norms writes inv_out (n) float64: one read of the table, no atomics.  Timing name: "similar_norms".
 *
 * poi_similar_topk: 1 <= k <= 32 (POI_ENOTSUP beyond: poi_similar_rows + poi_topk_select is the route for a larger k).  inv_norm (n)
 * from poi_row_inv_norms, or NULL: computed into the context's workspace inside the call - no cache is kept, so none can go stale.  A
 * workgroup keeps 32 query rows resident and streams the table's 32-row tiles past them (audience's walk); with g > 0 a pair whose
 * bound g + (1 - g) emb cannot enter its query's list is not given its distance - the listed bits do not depend on that.  Launch
 * regimes: at most "similar_rows_max" queries (default 1024) write their score rows into the context's workspace and select from them
 * (k <= n, the rows within "select_chunk_mb"); otherwise at most "similar_split_max" queries (default 16384) cut the rows into "similar_grid" slices
 * and merge, larger calls run one workgroup per query block.  The output is bitwise the same on every route, grid and regime, for a
 * query alone or among thousands; no float atomics.  poi_ctx_last_plan: "similar_path", "similar_splits", "similar_split_max".
 * Timing names: "similar_topk" (the call), inside it "similar_norms", "similar_walk" and "similar_merge", or "similar_rows" and
 * "topk_select".
 *
 * poi_similar_rows is the same walk with a store epilogue: scores_out[q * ld + j] = sim(queries[q], j) for j < n (ld >= n; the columns
 * beyond n are not written), -inf at the query's own column and in the whole row of a rejected query (counted once).  The large-k
 * route - poi_topk_select with k up to 4096 takes the exclusion lists itself; its count_out still counts the query's own row - and an
 * independent check of the fused entry.  Timing name: "similar_rows".
 *
 * poi_similar_nearest - "because you visited X": for every POI lists[r][i] >= 0 of row r (lists (n, k) int32 with -1 fill, k <= 32)
 * the POI of the row's history h_ids[h_off[r] .. h_off[r + 1]) (in the order given, duplicates allowed) it is most similar to.  The
 * similarity is poi_diverse_rerank's, in float64 throughout: sim = g geo + (1 - g) x_i . x_l / (|x_i| |x_l|) with float64 row
 * products and sqrt norms, 0 for a zero row; g in [0, 1] (a part with zero weight is not evaluated: its inputs may be NULL).  pos_out
 * (n, k) int32: the position INSIDE the row's history with the largest similarity, ties to the lower position; -1 for a -1 entry or
 * an empty history.  sim_out (n, k) float64 or NULL: that similarity, -inf there.  A listed id outside [-1, n_item), offsets out of
 * order or a history id outside [0, n_item) rejects the row: -1 / -inf, counted once.  It attributes a recommendation to the most
 * similar visited POI; it does not decompose the model's score.  One wave per row.  Timing name: "similar_nearest".  n = 0 is a no-op. */
int poi_row_inv_norms(poi_ctx* ctx, const float* x, int32_t n, int32_t dim, double* inv_out, void* stream);
int poi_similar_topk(poi_ctx* ctx, const float* x, int32_t n, int32_t dim, const double* coords, const double* cphi,
                     double geo_weight, double scale_km, const double* inv_norm,
                     const int32_t* queries, int32_t n_q, const int32_t* ex_off, const int32_t* ex, int32_t k,
                     int32_t* idx_out, float* score_out, int32_t* count_out, void* stream);
int poi_similar_rows(poi_ctx* ctx, const float* x, int32_t n, int32_t dim, const double* coords, const double* cphi,
                     double geo_weight, double scale_km, const double* inv_norm,
                     const int32_t* queries, int32_t n_q, float* scores_out, int64_t ld, void* stream);
int poi_similar_nearest(poi_ctx* ctx, const float* items, int32_t n_item, int32_t dim, const double* coords, const double* cphi,
                        double geo_weight, double scale_km,
                        const int32_t* lists, int32_t n, int32_t k, const int32_t* h_off, const int32_t* h_ids,
                        int32_t* pos_out, double* sim_out, void* stream);

/* ---- fold-in (additive to 9): a user row of OboBpr / OboVBpr for a check-in history the model never trained on -------------------------------
 * The factorisation family's only user representation is a trained row of ux (and ue).  Fold-in freezes the item side and runs the
 * model's own per-check-in SGD rule - public/BPR.py:216-230 (OboBpr.bpr_train: the ux[u] part of the update) and :287-306 (OboVBpr:
 * usr and use are regularised with the same lambda, :294-304, so [ux[u] | ue[u]] moves exactly like one BPR-MF user row against
 * [lt | fi ei^T]) - on one fresh row over that history.  For new user r with history p[off[r] .. off[r + 1]):
 *   w = w0[r] (zeros when w0 is NULL);  for e = 0 .. epochs - 1, for t in history order:
 *     d = Y[p_t] - Y[q_{e,t}],   x = w . d,   loss[r][e] += -log sigmoid(x)   (x before the update),
 *     w = w - alpha (-sigmoid(-x) d + lambda w)
 *   Y = items (n_item + 1, dim), float32 or a registered half table (the evaluation snapshot trained_items: dim = D for OboBpr, 2 D for
 *   OboVBpr); q_{e,t} = q[e * q_epoch_stride + off[r] + t] - q_epoch_stride = 0 reuses one draw for every epoch, the usual value is the
 *   total number of check-ins off[n].  Ids lie in [0, n_item] (the padding row is a legal id, as in poi_bpr_step).
 * Arithmetic: the running w, the dot product, the sigmoid and the loss are float64 (alpha and lambda are taken at their float values) and
 * are rounded to float32 once, at the end - the choice poi_session_advance makes for h.  Every sum has one fixed order (per lane its
 * columns ascending, then a fixed tree over 16 lanes); no atomics touch a result.  A user's output bits depend on its own history,
 * negatives and w0 alone: not on the other users of the call, on its position in the call or on the grid.
 * Edge cases: epochs = 0 or an empty history returns w0[r] (zeros without w0) and losses 0; p_t == q_t is legal (d = 0: only the decay
 * acts).  A user with off[r + 1] < off[r], off[r] < 0 or an id outside [0, n_item] among the ids it reads is a bad user: a NaN row, NaN
 * losses, counted once (poi_ctx_take_bad_ids), and nothing else moves.  The offsets themselves must lie inside p / q (the caller's
 * contract, as for every CSR argument).
 * w_out (n, dim) may alias w0; loss_out (n, epochs) or NULL.  dim: a multiple of 4, up to 256.  n = 0 is a no-op.
 * One kernel: a 16-lane row of a wave per user, the rows and ids of the next steps in flight while a step computes (foldin.hip).
 * Timing name: "foldin". */
int poi_foldin_bpr(poi_ctx* ctx, const float* items, int32_t n_item, int32_t dim,
                   const int32_t* off, const int32_t* p, const int32_t* q, int64_t q_epoch_stride,
                   int32_t n, int32_t epochs, float alpha, float lambda,
                   const float* w0, float* w_out, float* loss_out, void* stream);

/* ---- fold-in for the successive-POI models (additive to 9): a row of OboFpmc_lr's ui or of OboPrme's du for an unseen history --------------
 * FPMC-LR and PRME represent a user by one trained row.  With the item side frozen, each model's per-transition rule on that row is
 * poi_foldin_bpr's chain with two per-step scalars that do not depend on the row, a weight a and an offset c.  A history
 * p[off[r] .. off[r + 1]) of length L has the transitions t = 1 .. L - 1 with prev = p[t - 1], target p[t] and negative
 * q_{e,t} = q[e * q_epoch_stride + off[r] + t]; position 0 is no step.
 *   FPMC-LR (public/FPMC_LR.py:113-140, the ui part of the update, one negative per transition as the driver draws):
 *     c = ai[prev] . (ia[p_t] - ia[q]),   x = w . (iu[p_t] - iu[q]) + c,   w -= alpha (-sigmoid(-x) (iu[p_t] - iu[q]) + lambda w)
 *   PRME (public/PRME.py:173-214, the du part):
 *     far = gap_t > thd,  wgt = (1 + d_t)^0.25,  a = far ? 1 : wgt cw,  b = far ? 0 : wgt (1 - cw)
 *     c = b (|ds[q] - ds[prev]|^2 - |ds[p_t] - ds[prev]|^2),   x = a (|w - dp[q]|^2 - |w - dp[p_t]|^2) + c
 *     w += alpha (sigmoid(-x) 2 a (dp[p_t] - dp[q]) - lambda w)
 *   loss[r][e] += -log sigmoid(x) in both.  The reference's PRME step returns +log sigmoid(x) (as poi_prme_step does); fold-in keeps
 *   poi_foldin_bpr's sign for both models.  The reference's last-wins collapse of repeated rows concerns dp / ds only and does not
 *   touch the du row: p_t == q and p_t == prev are legal here, nothing but w moves.
 * Arithmetic: the running row, x, the sigmoid and the loss are float64 and are rounded to float32 once, at the end; alpha and lambda
 * enter at their float values, cw too.  Gathered rows are float32.  Every sum has one fixed order (per lane its columns ascending, then
 * a fixed tree over 16 lanes); no atomics touch a result; no output depends on the grid.
 *
 * The terms pass writes the scalars, float64, at the CSR position: c_out[e * q_epoch_stride + pos] (one epoch's worth when
 * q_epoch_stride = 0), a_out[pos] once per position; the first position of a history is written as 0.  total = the number of check-ins
 * (the length of p; off[n] for a well-formed CSR).  d_t is dist[pos] (float64 km) or, with dist NULL, cal_dis(cordi[p_t], cordi[prev]) in
 * float64 in cal_dis's operation order (cordi (n_item + 1, 2) lat, lon with the pad row, as poi_prme_score_all).  gap[pos]: minutes.
 * A negative id of -1 means "no negative exists" (poi_fpmc_sample_negatives emits it for a target without neighbours): the step is
 * skipped - no update, no decay, no loss - and its c is 0.  An entry with any other id outside [0, n_item], or with a distance that is
 * negative or not finite, becomes NaN; bad ids are not counted here - the chain counts its user.  With descending offsets the entries at
 * positions that two histories claim are unspecified.  Timing name: "foldin_terms". */
int poi_foldin_terms_fpmc(poi_ctx* ctx, const poi_fpmc_params* prm, const int32_t* off, const int32_t* p, const int32_t* q,
                          int64_t q_epoch_stride, int32_t n, int64_t total, int32_t epochs, double* c_out, void* stream);
int poi_foldin_terms_prme(poi_ctx* ctx, const poi_prme_params* prm, const double* cordi, const int32_t* off, const int32_t* p, const int32_t* q,
                          int64_t q_epoch_stride, const int32_t* gap, const double* dist, int32_t n, int64_t total, int32_t epochs,
                          int32_t threshold, float cw, double* a_out, double* c_out, void* stream);
/* The chain.  items (n_item + 1, dim) float32: iu for FPMC-LR, dp for PRME.  form: POI_FOLDIN_DOT x = w . d + c, gradient direction d;
 * POI_FOLDIN_METRIC x = a (|w - y_q|^2 - |w - y_p|^2) + c, evaluated as a sum of d (2 w - y_p - y_q), gradient direction 2 a d;
 * d = y_p - y_q.  first (0 or 1): the first position of a history that is a step.  a (per position) NULL means 1 and is not read in
 * the dot form, c NULL means 0; c of epoch e lies at c + e * c_epoch_stride.  With a = c = NULL, first = 0 and valid ids the dot form
 * performs poi_foldin_bpr's operations in its order: the same bits.
 * For new user r: w = w0[r] (zeros when w0 is NULL), then epochs x (L - first) steps in history order.  L <= first or epochs = 0
 * returns w0[r] and losses 0.  A step whose negative is -1 is skipped.  A user with off[r + 1] < off[r], off[r] < 0, any other id
 * outside [0, n_item] among the ids it reads (with first = 1 its first check-in included) or a term that is not finite is a bad user:
 * a NaN row, NaN losses, counted once (poi_ctx_take_bad_ids), and nothing else moves.  A user's output bits depend on its own history,
 * negatives, terms and w0 alone.  w_out (n, dim) may alias w0; loss_out (n, epochs) or NULL.  dim: a multiple of 4, up to 256.  n = 0 is
 * a no-op.  One kernel: a 16-lane row of a wave per user, the rows, ids and terms of the next steps in flight while a step computes
 * (foldin_seq.hip).  Timing name: "foldin_pair". */
enum { POI_FOLDIN_DOT = 0, POI_FOLDIN_METRIC = 1 };
int poi_foldin_pair(poi_ctx* ctx, const float* items, int32_t n_item, int32_t dim, int32_t form, int32_t first,
                    const int32_t* off, const int32_t* p, const int32_t* q, int64_t q_epoch_stride,
                    const double* a, const double* c, int64_t c_epoch_stride, int32_t n, int32_t epochs, float alpha, float lambda,
                    const float* w0, float* w_out, float* loss_out, void* stream);

/* ---- multi-GPU reconciliation (8e; new - the reference is single-process) ----------------------
 * Users are sharded across ranks, every rank trains on a full parameter replica with no data-path collective,
 * and replicas are reconciled ONCE PER EPOCH:  theta <- theta_start + combine(sum_r (theta_r - theta_start)),
 * one RCCL all-reduce over xGMI of ONE flat buffer (BASELINE.json north_star: "POI embedding table replicated and
 * kept consistent by an RCCL all-reduce once per epoch").
 *
 * elementwise helpers (kept from ABI 1): delta = cur - base ; cur = base + delta_sum */
int poi_delta_make(poi_ctx* ctx, const float* cur, const float* base, float* delta, int64_t n, void* stream);
int poi_delta_apply(poi_ctx* ctx, float* cur, const float* base, const float* delta_sum, int64_t n, void* stream);

/* The library's own RCCL communicator (librccl is bound with dlopen at first use: the .so loads without it).
 * Rank 0 calls poi_comm_unique_id and hands the 128 bytes to the other ranks over any host channel (bench.py:
 * one torch.distributed broadcast); every rank then calls poi_comm_init_rank (collective). */
#define POI_UNIQUE_ID_BYTES 128
typedef struct poi_comm poi_comm;
int poi_comm_available(void);          /* ABI 5: POI_OK when librccl can be bound in this process; makes no RCCL call (the probe of ranks != 0) */
int poi_comm_unique_id(char* id_host);
int poi_comm_init_rank(const char* id_host, int world, int rank, int device, poi_comm** out);
int poi_comm_destroy(poi_comm* comm);
int poi_comm_world(const poi_comm* comm);
int poi_comm_rank(const poi_comm* comm);

/* In-place SUM all-reduce of a device float buffer over the communicator (SURVEY.md 8b export list). */
int poi_allreduce_tables(poi_ctx* ctx, poi_comm* comm, float* buf, int64_t n, void* stream);

/* Per-epoch reconciliation object over a list of parameter tensors ("segments": rows x width floats, in place).
 * Combine rule per segment:
 *   POI_SYNC_SUM           theta_start + sum_r delta_r            every replica's epoch counts in full
 *   POI_SYNC_MEAN          theta_start + sum_r delta_r / world    model averaging
 *   POI_SYNC_MEAN_TOUCHED  per ROW: sum_r delta_r / #{r : replica r changed the row}  (the launch-level batch rule
 *                          one level up; a per-row flag travels in the same flat buffer)
 * All rules are the identity at world == 1.  poi_sync_end_epoch = make_delta + all-reduce + apply (the result
 * is also the next epoch's theta_start); the three steps are exported separately so that a host can run the
 * collective elsewhere (tests: gloo on CPU copies; single-GPU emulation of N replicas). */
enum { POI_SYNC_SUM = 0, POI_SYNC_MEAN = 1, POI_SYNC_MEAN_TOUCHED = 2 };
typedef struct poi_sync_seg { float* cur; int64_t rows; int64_t width; int32_t rule; int32_t dtype; /* POI_F32 | POI_F16 (cur holds IEEE half) */ } poi_sync_seg;
typedef struct poi_sync poi_sync;
int poi_sync_create(poi_ctx* ctx, int device, const poi_sync_seg* segs_host, int32_t n_seg, poi_sync** out);
int poi_sync_destroy(poi_sync* s);
int poi_sync_begin_epoch(poi_sync* s, void* stream);                  /* theta_start <- theta */
int poi_sync_make_delta(poi_sync* s, void* stream);                   /* flat buffer <- theta - theta_start | row flags */
int poi_sync_buffer(poi_sync* s, float** delta_dev, int64_t* n);      /* the flat buffer to SUM-all-reduce */
/* Segments stored as half (dtype POI_F16: config X's POI table) keep their snapshot as half - exact, the values are halves - and their
 * deltas as half in a SECOND flat buffer (n half elements, NULL / 0 without such segments), all-reduced as float16: the combined value is
 * rounded to half anyway, and a sum of `world` half deltas is off by at most world x 2^-11 of the DELTA (absolute) - below the 2^-11 of
 * the value that the final rounding costs wherever an epoch moves an element by less than its own magnitude.  Config X: 10 -> 5 GB of snapshot and 10 -> 5 GB per reconciliation.  poi_sync_end_epoch all-reduces both buffers;
 * callers that own the collective SUM-all-reduce this one too (element type float16).  The per-row touch counts stay in the float buffer. */
int poi_sync_buffer16(poi_sync* s, void** delta16_dev, int64_t* n);
int poi_sync_apply(poi_sync* s, int32_t world, void* stream);         /* theta <- theta_start + combine(buffer); theta_start <- theta */
int poi_sync_end_epoch(poi_sync* s, poi_comm* comm, void* stream);
int poi_sync_stats(poi_sync* s, double* allreduce_ms, int64_t* allreduce_bytes);   /* last end_epoch; synchronises */
const char* poi_sync_last_error(void);
/* out_dev[0] += 64-bit sum of the 32-bit patterns of x[0..n): replicas are bit-identical after a reconciliation
 * iff their checksums agree (caller zeroes out_dev). */
int poi_checksum(poi_ctx* ctx, const float* x, int64_t n, uint64_t* out_dev, void* stream);

/* ---- per-kernel timing with HIP events on the launch stream (bench.py's live roofline figures).
 * Kernel names: "seq_train", "rows_apply", "dense_apply", "seq_predict", "bpr_hogwild", "bpr_grad",
 * "bpr_apply", "score_topk", "score_all", "dist_prob", "sample_neg", "neg_dist", "carnn_train", "carnn_predict", "carnn_score", and for the tile engine "te_prep", "te_gather", "te_gemm_ax",
 * "te_rec_fwd", "te_head", "te_rec_bwd", "te_wgrad", "te_gemm_dx", "te_finalize", "te_predict".  poi_timing_get synchronises the device.
 * poi_timing_enable(ctx, N) with N > 1 instruments only every N-th training launch (poi_spatial_step / poi_gru_step): the event pairs
 * cost ~7 us of stream serialisation per kernel, and the sampled launches' average is the launch duration either way. */
int poi_timing_enable(poi_ctx* ctx, int on);
int poi_timing_reset(poi_ctx* ctx);
int poi_timing_get(poi_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);

/* ---- primitive self-test (wave reductions, atomics) used by tests/ and smoke() --------------- */
int poi_selftest(poi_ctx* ctx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POI_HIP_H */
