"""ctypes loader for the C ABI in include/somhip.h (libsomhip.so, built in-tree by `make lib`).

There is no Python or CPU fallback: if the library is missing, or no MI355X is visible
when an engine is created, the call raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOMHIP_LIB", os.path.join(HERE, "libsomhip.so"))   # override: A/B builds

c_float_p = C.POINTER(C.c_float)
c_i32_p = C.POINTER(C.c_int32)
c_i16_p = C.POINTER(C.c_int16)
c_u16_p = C.POINTER(C.c_uint16)
c_u8_p = C.POINTER(C.c_uint8)
c_u64_p = C.POINTER(C.c_uint64)
c_u32_p = C.POINTER(C.c_uint32)
c_i64_p = C.POINTER(C.c_int64)
c_double_p = C.POINTER(C.c_double)


class SomParams(C.Structure):
    _fields_ = [("length", C.c_int64), ("alpha", C.c_float), ("radius", C.c_float),
                ("alpha_type", C.c_int32), ("use_fixed", C.c_int32), ("use_weights", C.c_int32),
                ("batch", C.c_int64), ("start_iter", C.c_int64), ("count", C.c_int64),
                ("data_first", C.c_int64)]


class LvqParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("length", C.c_int64), ("alpha", C.c_float),
                ("alpha_type", C.c_int32), ("winlen", C.c_float), ("epsilon", C.c_float),
                ("start_iter", C.c_int64), ("count", C.c_int64), ("data_first", C.c_int64)]


class QualityTotals(C.Structure):
    _fields_ = [("searched", C.c_int64), ("topo_defined", C.c_int64), ("topo_errors", C.c_int64), ("qerror", C.c_float)]


class DistortionTotals(C.Structure):
    _fields_ = [("energy", C.c_double), ("scale", C.c_double), ("samples", C.c_uint64)]


class BatchmapParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("radius", C.c_float), ("start_epoch", C.c_int64), ("count", C.c_int64),
                ("first", C.c_int64), ("n", C.c_int64)]


class GlvqParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("start_epoch", C.c_int64), ("count", C.c_int64), ("first", C.c_int64), ("n", C.c_int64),
                ("alpha", C.c_float), ("sigmoid_beta", C.c_float)]


class NgParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("lambda0", C.c_double), ("lambda_end", C.c_double), ("ranks", C.c_int64),
                ("start_epoch", C.c_int64), ("count", C.c_int64), ("first", C.c_int64), ("n", C.c_int64)]


class GrlvqParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("start_epoch", C.c_int64), ("count", C.c_int64), ("first", C.c_int64), ("n", C.c_int64),
                ("alpha", C.c_float), ("sigmoid_beta", C.c_float), ("eps", C.c_float)]


class GmlvqParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("start_epoch", C.c_int64), ("count", C.c_int64), ("first", C.c_int64), ("n", C.c_int64),
                ("alpha", C.c_float), ("sigmoid_beta", C.c_float), ("eps", C.c_float), ("rank", C.c_int32)]


class RslvqParams(C.Structure):
    _fields_ = [("epochs", C.c_int64), ("start_epoch", C.c_int64), ("count", C.c_int64), ("first", C.c_int64), ("n", C.c_int64),
                ("alpha", C.c_float), ("sigma2", C.c_float)]


# name -> (restype, argtypes); exactly the symbols include/somhip.h declares
SIGNATURES = {
    "somhip_last_error": (C.c_char_p, []),
    "somhip_version": (C.c_int, []),
    "somhip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "somhip_engine_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "somhip_engine_destroy": (None, [C.c_void_p]),
    "somhip_engine_stream": (C.c_void_p, [C.c_void_p]),
    "somhip_engine_sync": (C.c_int, [C.c_void_p]),
    "somhip_engine_set_scan_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "somhip_engine_set_update_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "somhip_scan_stats": (C.c_int, [C.c_void_p, c_u64_p]),
    "somhip_lvq_stats": (C.c_int, [C.c_void_p, c_u64_p]),
    "somhip_column_sums": (C.c_int, [C.c_void_p, c_float_p, C.POINTER(C.c_int64)]),
    "somhip_column_minmax": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.POINTER(C.c_int64)]),
    "somhip_centered_products": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "somhip_qerror2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int64, c_float_p, c_i32_p]),
    "somhip_debug_prefilter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_float_p, c_float_p, c_i64_p]),
    "somhip_debug_level1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_float_p, c_u32_p, c_i64_p]),
    "somhip_debug_prepared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_u16_p, c_u16_p, c_float_p, c_float_p,
                                        c_u16_p, c_u16_p, c_u16_p, c_float_p, c_float_p, c_i32_p]),
    "somhip_debug_prepared_state": (C.c_int, [C.c_void_p, c_i32_p, c_u16_p, c_u16_p, c_float_p, c_float_p]),
    "somhip_debug_rerank_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_float_p, c_u64_p, c_u32_p,
                                            c_float_p, c_u32_p, c_u32_p, c_u32_p, C.c_int64, c_i64_p, c_u64_p, c_i64_p]),
    "somhip_debug_scan_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, c_i32_p]),
    "somhip_debug_update_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SomParams), C.c_int64, C.c_int64, C.c_int64,
                                           c_i32_p]),
    "somhip_debug_device_ptrs": (C.c_int, [C.c_void_p, C.c_void_p, c_u64_p]),
    "somhip_debug_lvq_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LvqParams), C.c_int, c_i32_p]),
    "somhip_debug_lvq_relation": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LvqParams), C.c_int64, C.c_int64, c_u64_p,
                                            c_float_p, c_float_p, c_float_p, c_u32_p, c_i32_p, c_i32_p, c_i32_p]),
    "somhip_debug_lvq_components": (C.c_int, [C.c_void_p, c_u32_p, C.c_int64, C.c_int, c_i32_p, c_i32_p, c_i32_p]),
    "somhip_codebook_create": (C.c_int, [C.c_void_p, c_float_p, c_i32_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                         C.POINTER(C.c_void_p)]),
    "somhip_shard_units": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_i64_p, c_i64_p]),
    "somhip_codebook_create_interleaved": (C.c_int, [C.c_void_p, c_float_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "somhip_codebook_download": (C.c_int, [C.c_void_p, c_float_p]),
    "somhip_codebook_upload": (C.c_int, [C.c_void_p, c_float_p]),
    "somhip_codebook_destroy": (None, [C.c_void_p]),
    "somhip_dataset_create": (C.c_int, [C.c_void_p, c_float_p, C.c_int64, C.c_int, c_u8_p, c_i32_p,
                                        c_i16_p, c_i16_p, C.POINTER(C.c_void_p)]),
    "somhip_dataset_generate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int64, C.c_int64, c_i32_p,
                                          C.POINTER(C.c_void_p)]),
    "somhip_dataset_wrap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                             C.POINTER(C.c_void_p)]),
    "somhip_dataset_download_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, c_float_p]),
    "somhip_dataset_destroy": (None, [C.c_void_p]),
    "somhip_find_winners": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                      c_i32_p, c_float_p, c_i32_p]),
    "somhip_knn_max": (C.c_int, []),
    "somhip_knn_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_knn_vote": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_i32_p, c_i32_p, c_i32_p, c_i32_p]),
    "somhip_knn_vote_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_map_quality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_u32_p, c_double_p, C.c_float,
                                     C.POINTER(QualityTotals)]),
    "somhip_map_quality_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_conn_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "somhip_conn_destroy": (None, [C.c_void_p]),
    "somhip_conn_clear": (C.c_int, [C.c_void_p]),
    "somhip_conn_size": (C.c_int, [C.c_void_p, c_i64_p, c_u64_p]),
    "somhip_conn_read": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, c_u32_p, c_u32_p, c_u64_p]),
    "somhip_map_connectivity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, c_u32_p, c_double_p,
                                          C.c_float, C.POINTER(QualityTotals)]),
    "somhip_conn_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_som_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SomParams), c_i32_p, c_float_p]),
    "somhip_som_batchmap": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BatchmapParams), c_float_p]),
    "somhip_debug_batchmap_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_u32_p, c_double_p]),
    "somhip_debug_batchmap_combine": (C.c_int, [C.c_void_p, C.c_float, c_u32_p, c_double_p]),
    "somhip_batchmap_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_batchmap_begin": (C.c_int, [C.c_void_p]),
    "somhip_batchmap_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "somhip_batchmap_finish": (C.c_int, [C.c_void_p, C.c_float, C.c_int64, C.c_int64, c_float_p]),
    "somhip_batchmap_end": (C.c_int, [C.c_void_p]),
    "somhip_batchmap_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_i64_p]),
    "somhip_glvq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GlvqParams), c_double_p, c_i64_p]),
    "somhip_debug_glvq_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int64, c_i32_p]),
    "somhip_debug_glvq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_float_p, c_i32_p, c_float_p,
                                           c_i32_p, c_i64_p]),
    "somhip_debug_glvq_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, c_double_p, c_double_p,
                                         c_double_p, c_double_p, c_u32_p, c_double_p, c_u32_p, c_double_p, c_i64_p]),
    "somhip_debug_glvq_update": (C.c_int, [C.c_void_p, C.c_float, C.c_int64, c_double_p, c_u32_p, c_double_p, c_u32_p]),
    "somhip_glvq_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_ng_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(NgParams), c_float_p]),
    "somhip_debug_ng_schedule": (C.c_int, [C.POINTER(NgParams), C.c_int64, C.c_int64, c_double_p, c_i32_p, c_double_p]),
    "somhip_debug_ng_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_i32_p, c_float_p]),
    "somhip_debug_ng_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, c_double_p, C.c_int64, c_u32_p,
                                       c_double_p, c_double_p]),
    "somhip_debug_ng_update": (C.c_int, [C.c_void_p, c_u32_p, c_double_p, c_double_p]),
    "somhip_ng_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_grlvq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GrlvqParams), c_float_p, c_double_p, c_i64_p]),
    "somhip_grlvq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_float_p, c_float_p, c_i32_p, c_float_p,
                                      c_i32_p]),
    "somhip_debug_grlvq_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, c_float_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_u32_p, c_double_p, c_u32_p, c_double_p, c_i64_p,
                                          c_double_p, c_double_p, c_double_p]),
    "somhip_debug_grlvq_update": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int64, c_float_p, c_double_p, c_u32_p,
                                            c_double_p, c_u32_p, c_double_p]),
    "somhip_grlvq_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_gmlvq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GmlvqParams), c_float_p, c_double_p, c_i64_p]),
    "somhip_gmlvq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_float_p, C.c_int32, c_float_p, c_i32_p,
                                      c_float_p, c_i32_p]),
    "somhip_gmlvq_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_float_p, C.c_int32, c_float_p]),
    "somhip_debug_gmlvq_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, c_float_p, C.c_int32, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_u32_p, c_double_p, c_u32_p, c_double_p, c_i64_p,
                                          c_double_p]),
    "somhip_debug_gmlvq_update": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int64, c_float_p, C.c_int32, c_double_p, c_u32_p,
                                            c_double_p, c_u32_p, c_double_p]),
    "somhip_gmlvq_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_distortion_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "somhip_distortion_destroy": (None, [C.c_void_p]),
    "somhip_distortion_clear": (C.c_int, [C.c_void_p]),
    "somhip_distortion_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "somhip_distortion_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, c_double_p, C.POINTER(DistortionTotals)]),
    "somhip_distortion_read": (C.c_int, [C.c_void_p, c_u32_p, c_double_p, c_double_p]),
    "somhip_debug_distortion_evaluate": (C.c_int, [C.c_void_p, C.c_float, c_u32_p, c_double_p, c_double_p, c_double_p,
                                                   C.POINTER(DistortionTotals)]),
    "somhip_distortion_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_som_batchmap_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BatchmapParams), C.c_void_p, c_float_p]),
    "somhip_mapset_create": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    "somhip_mapset_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p]),
    "somhip_mapset_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p]),
    "somhip_mapset_destroy": (None, [C.c_void_p]),
    "somhip_mapset_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SomParams), c_i32_p, c_float_p]),
    "somhip_mapset_winners": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_i32_p, c_float_p, c_i32_p]),
    "somhip_debug_mapset_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, c_i32_p]),
    "somhip_mapset_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
    "somhip_som_auto_batch": (C.c_int, [C.POINTER(SomParams), C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]),
    "somhip_lvq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LvqParams), c_float_p, c_i32_p,
                                   c_float_p]),
    "somhip_batch_winner_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "somhip_shard_exchange_available": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_shard_winner_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "somhip_shard_winner_refine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "somhip_shard_winner_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "somhip_batch_topk_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "somhip_merge_topk_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    "somhip_lvq_rates_upload": (C.c_int, [C.c_void_p, c_float_p]),
    "somhip_lvq_rates_download": (C.c_int, [C.c_void_p, c_float_p]),
    "somhip_lvq_batch_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "somhip_lvq_batch_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LvqParams), C.c_int64, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_i64_p, c_i32_p, c_float_p]),
    "somhip_comm_unique_id": (C.c_int, [C.c_void_p]),
    "somhip_comm_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "somhip_comm_create_sockets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "somhip_comm_allreduce_min_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_comm_allreduce_sum_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_comm_allreduce_min_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_comm_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_comm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "somhip_comm_destroy": (None, [C.c_void_p]),
    "somhip_som_batch_update": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SomParams), C.c_int64,
                                          C.c_int64, C.c_int64, C.c_void_p]),
    "somhip_sammon_zero_pairs": (C.c_int, [C.c_void_p, c_u32_p, C.c_int64, c_i64_p]),
    "somhip_sammon": (C.c_int, [C.c_void_p, C.c_int64, c_float_p, c_float_p, c_double_p]),
    "somhip_class_nearest_later": (C.c_int, [C.c_void_p, c_float_p, c_i32_p]),
    "somhip_umatrix": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_double_p]),
    "somhip_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p]),
    "somhip_device_alloc": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "somhip_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "somhip_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_copy_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "somhip_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "somhip_timing_select": (C.c_int, [C.c_void_p, C.c_uint64]),
    "somhip_timing_reset": (C.c_int, [C.c_void_p]),
    "somhip_kernel_count": (C.c_int, []),
    "somhip_kernel_name": (C.c_char_p, [C.c_int]),
    "somhip_timing_get": (C.c_int, [C.c_void_p, C.c_int, c_i64_p, c_double_p]),
}

# ... and exactly the symbols include/somhip_rslvq.h declares (batch Robust Soft LVQ, K13: the header somhip.h includes)
RSLVQ_SIGNATURES = {
    "somhip_rslvq_train": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RslvqParams), c_double_p, c_i64_p]),
    "somhip_rslvq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, c_double_p, c_i64_p, c_double_p]),
    "somhip_debug_rslvq_chunk": (C.c_int, [C.c_int64, c_i64_p, c_i64_p]),
    "somhip_debug_rslvq_posterior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_int64, c_double_p,
                                               c_double_p, c_i32_p, c_double_p]),
    "somhip_debug_rslvq_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, c_double_p, c_double_p,
                                          c_double_p]),
    "somhip_debug_rslvq_update": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int64, c_double_p, c_double_p]),
    "somhip_rslvq_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
}

# ... and exactly the symbols include/somhip_glvq_pieces.h declares (batch GLVQ, K9, over data in pieces and over ranks)
GLVQ_PIECES_SIGNATURES = {
    "somhip_glvq_begin": (C.c_int, [C.c_void_p]),
    "somhip_glvq_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float]),
    "somhip_glvq_finish": (C.c_int, [C.c_void_p, C.c_float, c_double_p, c_i64_p, c_i64_p]),
    "somhip_glvq_end": (C.c_int, [C.c_void_p]),
    "somhip_glvq_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_i64_p]),
    "somhip_glvq_train_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GlvqParams), C.c_void_p, c_double_p, c_i64_p]),
}

# ... and exactly the symbols include/somhip_ng_dense.h declares (dense batch neural gas, K10d)
NG_DENSE_SIGNATURES = {
    "somhip_ng_train_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(NgParams), c_float_p]),
    "somhip_debug_ng_dense_schedule": (C.c_int, [C.POINTER(NgParams), C.c_int64, C.c_int64, c_double_p, c_double_p]),
    "somhip_debug_ng_dense_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_i32_p, c_float_p]),
    "somhip_debug_ng_dense_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int64, c_double_p,
                                             c_double_p]),
    "somhip_ng_dense_timing": (C.c_int, [C.c_void_p, c_i64_p, c_double_p]),
}

# ... and exactly the symbols include/somhip_batchmap_missing.h declares (the batch map over data with missing values, K8m)
BATCHMAP_MISSING_SIGNATURES = {
    "somhip_som_batchmap_missing": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BatchmapParams), c_float_p]),
    "somhip_debug_batchmap_missing_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_double_p, c_double_p]),
    "somhip_debug_batchmap_missing_combine": (C.c_int, [C.c_void_p, C.c_float, c_double_p, c_double_p]),
    "somhip_batchmap_missing_begin": (C.c_int, [C.c_void_p]),
    "somhip_batchmap_missing_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "somhip_batchmap_missing_finish": (C.c_int, [C.c_void_p, C.c_float, C.c_int64, C.c_int64, c_float_p]),
    "somhip_batchmap_missing_end": (C.c_int, [C.c_void_p]),
    "somhip_batchmap_missing_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_i64_p]),
}

_lib = None


def load():
    """Load libsomhip.so (no GPU needed for loading; creating an engine needs one)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not built -- run `make lib` (python -c 'import __graft_entry__ as g; "
                               "g.build()'); there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(RSLVQ_SIGNATURES.items()) + list(GLVQ_PIECES_SIGNATURES.items()) + \
                list(NG_DENSE_SIGNATURES.items()) + list(BATCHMAP_MISSING_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class SomhipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise SomhipError(load().somhip_last_error().decode())
