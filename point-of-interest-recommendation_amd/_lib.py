"""ctypes binding of libpoi_hip.so (include/poi_hip.h).  The library is the product: if it is not
built, or a call fails, this module raises - there is no CPU fallback."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p, POINTER

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpoi_hip.so")
ABI_VERSION = 9
P2V_FOLD_SPAN = 256        # items per softmax partial of poi_foldin_p2v (csrc/poi_kernels.h; checked against the library on load)

BPR_SNAPSHOT, BPR_HOGWILD = 0, 1


class PoiError(RuntimeError):
    pass


class GruParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("lt", "di", "ui", "wh", "bi", "vs", "bs", "wd", "lw")] + \
               [("n_item", c_int32), ("n_dist", c_int32), ("dim", c_int32)]


class CarnnParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("lt", "wd", "M")] + [("n_item", c_int32), ("n_dist", c_int32), ("dim", c_int32)]


class FpmcParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ui", "iu", "ia", "ai")] + [("n_user", c_int32), ("n_item", c_int32), ("dim", c_int32)]


class PrmeParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("du", "dp", "ds")] + [("n_user", c_int32), ("n_item", c_int32), ("dim", c_int32)]


class GeoieParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("g", "h", "t", "z", "ab")] + [("n_user", c_int32), ("n_item", c_int32), ("dim", c_int32)]


class Poi2vecParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("xu", "wl", "pb", "routes", "lrs", "probs", "rid")] + [(n, c_int32) for n in ("n_user", "n_item", "n_node", "depth", "dim")]


class CellParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("lt", "ui", "wh", "bi")] + [("n_item", c_int32), ("dim", c_int32), ("cell", c_int32)]


class VbprParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ux", "lt", "ue", "ei", "fi")] + [(n, c_int32) for n in ("n_user", "n_item", "dim", "n_img")]


FOLDIN_DOT, FOLDIN_METRIC = 0, 1    # POI_FOLDIN_*: the form of poi_foldin_pair
CELL_RNN, CELL_LSTM = 1, 4          # POI_CELL_*: the number of gate blocks


class SyncSeg(ctypes.Structure):
    _fields_ = [("cur", c_void_p), ("rows", c_int64), ("width", c_int64), ("rule", c_int32), ("dtype", c_int32)]


SYNC_SUM, SYNC_MEAN, SYNC_MEAN_TOUCHED = 0, 1, 2


class SeqTables(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("off", "p", "q", "dp", "dq")] + \
               [("n_user", c_int32), ("len_max", c_int32), ("max_len", c_int32)]


# name -> (restype, argtypes); mirrors include/poi_hip.h one to one (checked by tests/test_abi.py)
SIGNATURES = {
    "poi_abi_version": (c_int, []),
    "poi_ctx_create": (c_int, [POINTER(c_void_p), c_int]),
    "poi_ctx_destroy": (c_int, [c_void_p]),
    "poi_last_error": (c_char_p, [c_void_p]),
    "poi_ctx_num_cu": (c_int, [c_void_p]),
    "poi_ctx_set_engine": (c_int, [c_void_p, c_int]),
    "poi_ctx_set_batch_cap": (c_int, [c_void_p, c_float]),
    "poi_ctx_set_graph": (c_int, [c_void_p, c_int, c_int, c_int]),
    "poi_ctx_set_topk_seed": (c_int, [c_void_p, c_void_p, c_int32]),
    "poi_ctx_set_topk_filter": (c_int, [c_void_p, c_int]),
    "poi_ctx_topk_filter_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "poi_ctx_graph_replays": (c_int64, [c_void_p]),
    "poi_ctx_last_plan": (c_int, [c_void_p, c_char_p, POINTER(c_int64)]),
    "poi_ctx_take_bad_ids": (c_int64, [c_void_p, c_void_p]),
    "poi_ctx_register_f16": (c_int, [c_void_p, c_void_p, c_int64]),
    "poi_ctx_unregister_f16": (c_int, [c_void_p, c_void_p]),
    "poi_ctx_set_f16_rounding": (c_int, [c_void_p, c_int, ctypes.c_uint32]),
    "poi_ctx_set_split_products": (c_int, [c_void_p, c_int]),
    "poi_ctx_set_exact_forward": (c_int, [c_void_p, c_int, c_int]),
    "poi_ctx_set_option": (c_int, [c_void_p, ctypes.c_char_p, c_int]),
    "poi_ctx_set_small_launch": (c_int, [c_void_p, c_int]),
    "poi_ctx_set_one_sequence_path": (c_int, [c_void_p, c_int]),
    "poi_ctx_set_regroup_min": (c_int, [c_void_p, c_int]),
    "poi_bpr_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                             c_int32, c_float, c_float, c_void_p, c_int, c_void_p]),
    "poi_spatial_step": (c_int, [c_void_p, POINTER(GruParams), POINTER(SeqTables), c_void_p, c_int32, c_float, c_float,
                                 c_void_p, c_void_p]),
    "poi_gru_step": (c_int, [c_void_p, POINTER(GruParams), POINTER(SeqTables), c_void_p, c_int32, c_float, c_float,
                             c_void_p, c_void_p]),
    "poi_gru_predict": (c_int, [c_void_p, POINTER(GruParams), POINTER(SeqTables), c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                c_void_p]),
    "poi_carnn_step": (c_int, [c_void_p, POINTER(CarnnParams), POINTER(SeqTables), c_void_p, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "poi_carnn_predict": (c_int, [c_void_p, POINTER(CarnnParams), POINTER(SeqTables), c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_carnn_score_all": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                    c_int32, c_int32, c_double, c_void_p, c_void_p]),
    "poi_score_all": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "poi_score_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                               c_void_p, c_void_p, c_void_p]),
    "poi_topk": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "poi_auc_preference": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                   c_void_p, c_void_p]),
    "poi_sumsq": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "poi_dist_prob": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double,
                              c_void_p, c_void_p]),
    "poi_ulptai_build": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double,
                                 c_void_p, c_int32, c_void_p]),
    "poi_score_topk_ulptai": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                      c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "poi_score_topk_geo": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int32, c_double, c_int32, c_void_p, c_void_p, c_void_p]),
    "poi_rank_metrics": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_sample_negatives": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint64,
                                     c_void_p, c_void_p, c_void_p]),
    "poi_neg_dist_bins": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_double,
                                  c_void_p, c_void_p]),
    "poi_fpmc_neighbor_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_double, c_void_p, c_void_p]),
    "poi_fpmc_neighbor_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "poi_fpmc_sample_negatives": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int64, ctypes.c_uint64, c_void_p, c_void_p]),
    "poi_fpmc_step": (c_int, [c_void_p, POINTER(FpmcParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_void_p,
                              c_void_p]),
    "poi_prme_step": (c_int, [c_void_p, POINTER(PrmeParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_float,
                              c_float, c_int32, c_float, c_void_p, c_void_p]),
    "poi_prme_score_all": (c_int, [c_void_p, POINTER(PrmeParams), c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p, c_void_p]),
    "poi_prme_score_topk": (c_int, [c_void_p, POINTER(PrmeParams), c_void_p, c_void_p, c_void_p, c_int32, c_float, c_int32, c_void_p, c_void_p,
                                    c_void_p]),
    "poi_geoie_step": (c_int, [c_void_p, POINTER(GeoieParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64,
                               c_float, c_float, c_double, c_void_p, c_void_p]),
    "poi_geoie_pair_distances": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                         c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "poi_geoie_user_vectors": (c_int, [c_void_p, POINTER(GeoieParams), c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "poi_geoie_score_all_geo": (c_int, [c_void_p, POINTER(GeoieParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                        c_double, c_void_p, c_void_p]),
    "poi_geoie_score_topk_geo": (c_int, [c_void_p, POINTER(GeoieParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                         c_double, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_poi2vec_step": (c_int, [c_void_p, POINTER(Poi2vecParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64,
                                 c_int32, c_float, c_float, c_void_p, c_void_p]),
    "poi_poi2vec_scores": (c_int, [c_void_p, POINTER(Poi2vecParams), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                   c_void_p]),
    "poi_poi2vec_topk": (c_int, [c_void_p, POINTER(Poi2vecParams), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                 c_void_p, c_void_p, c_void_p]),
    "poi_poi2vec_topk_ex": (c_int, [c_void_p, POINTER(Poi2vecParams), c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                    c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_foldin_p2v": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "poi_foldin_p2v_span": (c_int, []),
    "poi_cell_step": (c_int, [c_void_p, POINTER(CellParams), POINTER(SeqTables), c_void_p, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "poi_cell_predict": (c_int, [c_void_p, POINTER(CellParams), POINTER(SeqTables), c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_vbpr_step": (c_int, [c_void_p, POINTER(VbprParams), c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_float, c_void_p, c_void_p]),
    "poi_vbpr_items": (c_int, [c_void_p, POINTER(VbprParams), c_void_p, c_void_p]),
    "poi_vbpr_users": (c_int, [c_void_p, POINTER(VbprParams), c_void_p, c_void_p]),
    "poi_session_advance": (c_int, [c_void_p, POINTER(GruParams), c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                    c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "poi_session_sts": (c_int, [c_void_p, POINTER(GruParams), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_explain_loo": (c_int, [c_void_p, POINTER(GruParams), c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "poi_session_cell_advance": (c_int, [c_void_p, POINTER(CellParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                         c_void_p]),
    "poi_session_carnn_advance": (c_int, [c_void_p, POINTER(CarnnParams), c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_int32,
                                          c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_score_topk_near": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int32, c_double, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_rank_scores": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_group_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int32, c_double, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_group_topk_scores": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "poi_route_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_double, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "poi_route_merge": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "poi_diverse_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_double, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_diverse_rerank": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_double,
                                   c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_diverse_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_double, c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int32, c_double, c_void_p, c_int64, c_void_p]),
    "poi_topk_select": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_audience": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int32, c_double, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_audience_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int32, c_double, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "poi_row_inv_norms": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "poi_similar_topk": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p, c_int32, c_void_p,
                                 c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_similar_rows": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p, c_int32, c_void_p,
                                 c_int64, c_void_p]),
    "poi_similar_nearest": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_double, c_double, c_void_p, c_int32, c_int32, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_candidates": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int32, c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_lists_chunk": (c_int, []),
    "poi_score_lists": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int32, c_double, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "poi_rerank_lists": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_double, c_double, c_int32, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "poi_rerank": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_int32, c_double, c_void_p, c_void_p, c_int32, c_void_p, c_double, c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p]),
    "poi_filter_build": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                 c_int64, c_void_p, c_void_p]),
    "poi_score_topk_filtered": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int32, c_double, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_double, c_void_p, c_void_p, c_int32,
                                        c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_topk_filtered_scores": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_labels_build": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "poi_score_topk_capped": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_double, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_topk_capped_scores": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                       c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_score_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_double, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    "poi_score_topk_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_double, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_labels_scores": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "poi_foldin_bpr": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float, c_float,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_foldin_terms_fpmc": (c_int, [c_void_p, POINTER(FpmcParams), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64, c_int32, c_void_p, c_void_p]),
    "poi_foldin_terms_prme": (c_int, [c_void_p, POINTER(PrmeParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64,
                                      c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p]),
    "poi_foldin_pair": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                c_int32, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "poi_delta_make": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "poi_delta_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "poi_comm_available": (c_int, []),
    "poi_comm_unique_id": (c_int, [c_void_p]),
    "poi_comm_init_rank": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_void_p)]),
    "poi_comm_destroy": (c_int, [c_void_p]),
    "poi_comm_world": (c_int, [c_void_p]),
    "poi_comm_rank": (c_int, [c_void_p]),
    "poi_allreduce_tables": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "poi_sync_create": (c_int, [c_void_p, c_int, POINTER(SyncSeg), c_int32, POINTER(c_void_p)]),
    "poi_sync_destroy": (c_int, [c_void_p]),
    "poi_sync_begin_epoch": (c_int, [c_void_p, c_void_p]),
    "poi_sync_make_delta": (c_int, [c_void_p, c_void_p]),
    "poi_sync_buffer": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "poi_sync_buffer16": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "poi_sync_apply": (c_int, [c_void_p, c_int32, c_void_p]),
    "poi_sync_end_epoch": (c_int, [c_void_p, c_void_p, c_void_p]),
    "poi_sync_stats": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "poi_sync_last_error": (c_char_p, []),
    "poi_checksum": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "poi_timing_enable": (c_int, [c_void_p, c_int]),
    "poi_timing_reset": (c_int, [c_void_p]),
    "poi_timing_get": (c_int, [c_void_p, c_char_p, POINTER(c_double), POINTER(c_int64)]),
    "poi_selftest": (c_int, [c_void_p, c_void_p]),
}

_lib = None


def load():
    """dlopen the in-tree library and bind every exported symbol.  Raises PoiError when missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PoiError("%s is not built - run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(no CPU fallback exists for the hot path)" % LIB_PATH)
    # PyTorch is the device-memory container: its HIP runtime (torch/lib/libamdhip64.so) must be the one this
    # library binds to - loading libpoi_hip.so first would pull in a second runtime from /opt/rocm, which
    # knows nothing about torch's allocations and streams ("no HIP device visible").
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError -> missing export
        fn.restype = res
        fn.argtypes = args
    if lib.poi_abi_version() != ABI_VERSION:
        raise PoiError("libpoi_hip.so ABI %d != binding %d" % (lib.poi_abi_version(), ABI_VERSION))
    if lib.poi_foldin_p2v_span() != P2V_FOLD_SPAN:
        raise PoiError("libpoi_hip.so folds POI2Vec in spans of %d, the binding expects %d" % (lib.poi_foldin_p2v_span(), P2V_FOLD_SPAN))
    _lib = lib
    return lib


# keys of poi_ctx_last_plan (include/poi_hip.h)
PLAN_KEYS = ("tile", "one", "rec1", "xrec1", "hyb", "bintab", "ppoi", "listed", "fwd_tab", "xft", "xcomp", "head_split", "efuse", "early_bins",
             "fork", "hyb_fwd_seq", "hyb_fwd_wg", "hyb_bwd_seq", "hyb_bwd_wg", "cell_kernel", "cell_grid", "session_path", "session_tiles", "session_tile_min",
             "near_path", "near_splits", "near_split_max", "rank_splits", "geoie_score_span", "geoie_score_splits",
             "group_path", "group_splits", "group_split_max", "route_path", "route_splits",
             "diverse_path", "diverse_splits", "diverse_split_max",
             "select_rows_per_chunk", "select_chunks", "select_path", "select_splits", "xfwd_ids_lds", "stream_hints",
             "filter_path", "filter_splits", "filter_split_max", "audience_path", "audience_splits", "audience_split_max",
             "similar_path", "similar_splits", "similar_split_max", "capped_splits", "capped_split_max", "lists_path",
             "labels_splits", "labels_split_max", "labels_home", "labels_chunks", "labels_rows_per_chunk",
             "explain_columns", "explain_tiles", "explain_start")


class Context:
    """Owns one poi_ctx (device scratch + error text) bound to a HIP device."""

    def __init__(self, device=0):
        self.lib = load()
        h = c_void_p()
        rc = self.lib.poi_ctx_create(ctypes.byref(h), int(device))
        if rc != 0:
            raise PoiError("poi_ctx_create(%d) failed: %s" % (device, self.lib.poi_last_error(None).decode()))
        self.handle = h
        self.device = int(device)
        self.options = {}           # name -> value of every set_option() so far

    def check(self, rc):
        if rc != 0:
            raise PoiError("libpoi_hip error %d: %s" % (rc, self.lib.poi_last_error(self.handle).decode()))

    @property
    def num_cu(self):
        return self.lib.poi_ctx_num_cu(self.handle)

    def set_engine(self, name):
        """'auto' | 'seq' | 'tile' | 'tile32' | 'exact' (float64 arithmetic; see poi_ctx_set_engine)."""
        self.check(self.lib.poi_ctx_set_engine(self.handle, {"auto": 0, "seq": 1, "tile": 2, "tile32": 3, "exact": 4}[name]))

    def set_graph(self, on, min_n=0, max_n=1 << 30):
        """hipGraph replay of the tile engine's training launches (poi_ctx_set_graph)."""
        self.check(self.lib.poi_ctx_set_graph(self.handle, int(bool(on)), int(min_n), int(max_n)))

    def set_topk_seed(self, seed, k_seed):
        """Seed ids of the next fused top-K call (poi_ctx_set_topk_seed): an (n, k_seed) int32 device tensor or None."""
        self.check(self.lib.poi_ctx_set_topk_seed(self.handle, None if seed is None else seed.data_ptr(), int(k_seed)))

    def set_topk_filter(self, on):
        """Two-stage fused top-K (f16 filter + exact float32 rescoring): poi_ctx_set_topk_filter.  on: False / True, or "items" / "users" =
        two-stage with the item-stationary GEO filter forced / forbidden (default: chosen by shape)."""
        mode = {"items": 2, "users": 3}.get(on, int(bool(on))) if isinstance(on, str) else int(bool(on))
        self.check(self.lib.poi_ctx_set_topk_filter(self.handle, mode))

    def topk_filter_stats(self):
        """dict(users, survivors, tiles, tiles_flagged) of the last two-stage fused top-K call (poi_ctx_topk_filter_stats)."""
        v = [c_int64(0) for _ in range(4)]
        self.check(self.lib.poi_ctx_topk_filter_stats(self.handle, *[ctypes.byref(x) for x in v]))
        return dict(zip(("users", "survivors", "tiles", "tiles_flagged"), (x.value for x in v)))

    def take_bad_ids(self, stream=None):
        """Out-of-range ids seen by poi_bpr_step (rejected transitions of poi_fpmc_step / poi_prme_step) since the last call (synchronises the stream, clears the counter)."""
        v = int(self.lib.poi_ctx_take_bad_ids(self.handle, ctypes.c_void_p(stream or 0)))
        if v < 0:
            self.check(v)
        return v

    def graph_replays(self):
        return int(self.lib.poi_ctx_graph_replays(self.handle))

    def last_plan(self, key=None):
        """The plan the last poi_spatial_step / poi_gru_step on this context took (poi_ctx_last_plan): the value of `key` (one of
        PLAN_KEYS), or a dict of every key when key is None.  The hyb_* keys synchronise the launch stream."""
        if key is None:
            return {k: self.last_plan(k) for k in PLAN_KEYS}
        v = c_int64(0)
        self.check(self.lib.poi_ctx_last_plan(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_batch_cap(self, cap):
        """Batch rule cap (include/poi_hip.h, poi_ctx_set_batch_cap): 1 = mean rule, 0 = the mini-batch rule of public/GRU.py:395-498."""
        self.check(self.lib.poi_ctx_set_batch_cap(self.handle, float(cap)))
        self.batch_cap = float(cap)

    def register_f16(self, tensor):
        """Declare a torch.float16 device tensor as an IEEE-half POI table (poi_ctx_register_f16)."""
        self.check(self.lib.poi_ctx_register_f16(self.handle, tensor.data_ptr(), tensor.numel() * 2))

    def set_f16_rounding(self, mode, seed=0):
        """'nearest' | 'stochastic' write-back of a half POI table (poi_ctx_set_f16_rounding)."""
        self.check(self.lib.poi_ctx_set_f16_rounding(self.handle, {"nearest": 0, "stochastic": 1}[mode], int(seed) & 0xFFFFFFFF))

    def set_split_products(self, on=True):
        """Recurrent kernels of the tile engine on bf16 x 3 split products (default) or float32-input MFMAs (poi_ctx_set_split_products)."""
        self.check(self.lib.poi_ctx_set_split_products(self.handle, 1 if on else 0))

    def set_exact_forward(self, on=True, per_sequence_max=-1):
        """Training launches run the forward pass in fixed point on the int8 matrix cores + float64 gates (poi_ctx_set_exact_forward, default
        on); per_sequence_max: launches of at most this many sequences use the per-sequence float64 kernel (default 512; -1 keeps it)."""
        self.check(self.lib.poi_ctx_set_exact_forward(self.handle, 1 if on else 0, int(per_sequence_max)))

    def set_option(self, name, value):
        """Named tuning switch of the tile engine (poi_ctx_set_option: "forward_table_compact", "forward_table_compact_min", "xfwd_ids_lds", "stream_hints", "stream_hints_min", "head_split",
        "early_bins", "hot_bins", "hybrid", "hybrid_min", "hybrid_max", "hybrid_force"; "cell_grid" of poi_cell_step; "session_tile_min" of poi_session_advance;
        "near_split_max" / "near_grid" of poi_score_topk_near; "rank_grid" of poi_score_rank; "geoie_score_span" of
        poi_geoie_score_all_geo / poi_geoie_score_topk_geo; "group_split_max" / "group_grid" of poi_group_topk; "route_split_max" / "route_grid" of
        poi_route_expand; "diverse_split_max" / "diverse_grid" of poi_diverse_pool / poi_diverse_topk; "select_split_max" /
        "select_grid" / "select_chunk_mb" of poi_topk_select / poi_score_candidates; "filter_split_max" / "filter_grid" / "filter_gather_cost" of
        poi_score_topk_filtered; "audience_split_max" / "audience_grid" of poi_score_audience / poi_audience_rows; "similar_split_max" /
        "similar_grid" / "similar_rows_max" of poi_similar_topk / poi_similar_rows; "capped_split_max" / "capped_grid" of
        poi_score_topk_capped, "capped_hist_kb" of poi_labels_build; "labels_split_max" / "labels_grid" / "labels_lds_kb" / "labels_ws_kb" of
        poi_score_labels / poi_score_topk_labels / poi_labels_scores; "explain_start" of poi_explain_loo).  `options` keeps what was set."""
        self.check(self.lib.poi_ctx_set_option(self.handle, name.encode(), int(value)))
        self.options[name] = int(value)

    def set_small_launch(self, max_sequences=1800):
        """Launches of at most this many sequences use the per-sequence recurrent kernels (poi_ctx_set_small_launch; 0 disables)."""
        self.check(self.lib.poi_ctx_set_small_launch(self.handle, int(max_sequences)))

    def set_regroup_min(self, min_sequences=1280):
        """Launches below this many sequences take the two-table path instead of the regrouped backward pass (poi_ctx_set_regroup_min)."""
        self.check(self.lib.poi_ctx_set_regroup_min(self.handle, int(min_sequences)))

    def set_one_sequence_path(self, on=True):
        """Launches of one Distance2Pre sequence through the five-kernel path (poi_ctx_set_one_sequence_path)."""
        self.check(self.lib.poi_ctx_set_one_sequence_path(self.handle, 1 if on else 0))

    def unregister_f16(self, tensor):
        self.check(self.lib.poi_ctx_unregister_f16(self.handle, tensor.data_ptr()))

    def timing(self, on=True, period=1):
        """Per-kernel HIP-event timing; period N > 1 instruments only every N-th training launch (poi_timing_enable)."""
        self.check(self.lib.poi_timing_reset(self.handle))
        self.check(self.lib.poi_timing_enable(self.handle, (max(int(period), 1) if on else 0)))

    def timing_get(self, kernel):
        """(total milliseconds, launches) recorded for `kernel` since the last timing() call."""
        ms, n = c_double(0), c_int64(0)
        self.check(self.lib.poi_timing_get(self.handle, kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.poi_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts = {}


def context(device=0):
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]
