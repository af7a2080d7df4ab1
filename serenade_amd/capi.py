"""ctypes binding of libserenade_hip.so (include/serenade_hip.h).  Thin: every call maps 1:1 onto a C
entry point and raises SerenadeError with srn_last_error() on a negative return code."""
import ctypes as C
import os

import numpy as np

from . import build as _build

SRN_OK, SRN_EINVAL, SRN_ENOMEM, SRN_EHIP, SRN_ERANGE, SRN_EIO, SRN_ENODEV, SRN_ESTATE, SRN_ETIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7, -8
ATTR_ADULT, ATTR_FOR_SALE, ATTR_NONE = 1, 2, 0xFF
FLAG_BUSINESS_LOGIC = 1
MAX_HOW_MANY, MAX_SESSION_LEN, MAX_K = 512, 255, 8192

_CODES = {SRN_EINVAL: "SRN_EINVAL", SRN_ENOMEM: "SRN_ENOMEM", SRN_EHIP: "SRN_EHIP", SRN_ERANGE: "SRN_ERANGE",
          SRN_EIO: "SRN_EIO", SRN_ENODEV: "SRN_ENODEV", SRN_ESTATE: "SRN_ESTATE", SRN_ETIMEOUT: "SRN_ETIMEOUT"}


class SerenadeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_CODES.get(code, code), msg))
        self.code = code


class SessionsView(C.Structure):
    _fields_ = [("sess_off", C.c_void_p), ("items", C.c_void_p), ("max_ts", C.c_void_p), ("n_sessions", C.c_size_t)]


class IndexInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_items", "n_sessions_total", "n_sessions_kept", "nnz_rows", "nnz_postings",
                                          "m_index", "max_session_len", "max_row_len", "device_bytes")] + \
               [("device", C.c_int32), ("offsets_64bit", C.c_int32), ("idf_weighting", C.c_double), ("incomplete_items", C.c_uint64)]


class IndexHostState(C.Structure):   # srn_index_host_state_t
    _fields_ = [("host_complete", C.c_int32), ("reserved", C.c_int32), ("build_bytes_on_device", C.c_uint64), ("materialisations", C.c_uint64)] + \
               [(n, C.c_double) for n in ("ms_upload", "ms_group", "ms_quantile", "ms_build", "ms_items", "ms_attach", "ms_materialize")]


class ShardGroupStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_shards", "batches", "queries", "bytes_head", "bytes_counts", "bytes_lists", "bytes_results", "bytes_lists_max_rank")] + \
               [("transport", C.c_uint32), ("overlapped", C.c_uint32)] + [(n, C.c_uint64) for n in ("stage_batches", "bytes_stage_candidates", "bytes_stage_minpos", "neighbour_batches", "bytes_neighbours")]


# srn_shard_comm_t: the application's transport for a shard group (three collectives on device buffers)
ALL_REDUCE_MAX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
ALL_GATHER_V_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p)


class ShardComm(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_reduce_max_i32", ALL_REDUCE_MAX_FN), ("all_gather", ALL_GATHER_FN), ("all_gather_v", ALL_GATHER_V_FN),
                ("all_reduce_min_i32", ALL_REDUCE_MAX_FN)]


SHARD_GROUP_ID_BYTES = 256
FLAG_INPUTS_RESIDENT = 2
FLAG_EXCLUDE_SESSION = 4
FLAG_EXCLUDE_SEEN = 8
FLAG_FILL = 16
FLAG_EVAL_HANDLER = 32
MAX_FALLBACK = 4096
TRENDING_POPULAR_TAIL = 1


class EvalTrial(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("k", "m", "how_many", "max_items_in_session", "length", "flags", "max_chunk_queries", "history")]


class EvalResult(C.Structure):
    _fields_ = [("n_evaluations", C.c_uint64)] + \
               [(n, C.c_double) for n in ("mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score",
                                          "sum_mrr", "sum_ndcg", "sum_hit_rate", "sum_popularity", "sum_precision", "sum_recall")] + \
               [("covered_items", C.c_uint64), ("unique_training_items", C.c_uint64), ("ms_predict", C.c_double), ("ms_eval", C.c_double)]


MAX_BOOTSTRAP, BOOTSTRAP_SUMS = 4096, 7


class Bootstrap(C.Structure):   # srn_bootstrap_t
    _fields_ = [("seed", C.c_uint64), ("replicates", C.c_uint32), ("flags", C.c_uint32)]


MAX_SEGMENTS = 64
SEG_STATE, SEG_LABEL, SEG_TARGET_COUNT, SEG_CURRENT_COUNT = 1, 2, 3, 4


class Segments(C.Structure):   # srn_segments_t
    _fields_ = [("mode", C.c_uint32), ("segments", C.c_uint32), ("labels", C.c_void_p), ("n_labels", C.c_size_t), ("bounds", C.c_void_p), ("reserved", C.c_uint64)]


class EvalSegment(C.Structure):   # srn_eval_segment_t
    _fields_ = [("n_evaluations", C.c_uint64)] + [(n, C.c_double) for n in ("sum_mrr", "sum_ndcg", "sum_hit_rate", "sum_popularity", "sum_precision", "sum_recall")]


class LoadInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("lines", "rows", "skipped", "host_parsed")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_upload", "ms_parse", "ms_group", "ms_download")]


EVENTS_TIME_I64, EVENTS_DEVICE = 1, 2
SPLIT_TRAIN, SPLIT_TEST, SPLIT_OUT, SPLIT_RARE, SPLIT_SHORT_TRAIN, SPLIT_UNKNOWN, SPLIT_SHORT_TEST = 1, 2, 16, 17, 18, 19, 20
SPLIT_TEST_KNOWN_ITEMS = 1
SPLIT_NO_POS = 0xFFFFFFFF


class EventsView(C.Structure):   # srn_events_view_t
    _fields_ = [("session_ids", C.c_void_p), ("item_ids", C.c_void_p), ("times", C.c_void_p), ("n", C.c_size_t), ("device", C.c_int32), ("reserved", C.c_int32)]


class Split(C.Structure):   # srn_split_t
    _fields_ = [("cutoff", C.c_uint64), ("start", C.c_uint64), ("end", C.c_uint64)] + \
               [(n, C.c_uint32) for n in ("min_item_support", "min_session_len", "flags", "reserved")]


class SplitInfo(C.Structure):   # srn_split_info_t
    _fields_ = [(n, C.c_uint64) for n in ("train_rows", "train_sessions", "train_items", "test_rows", "test_sessions", "test_items", "dropped_out", "dropped_rare",
                                          "dropped_short_train", "dropped_unknown", "dropped_short_test", "sessions", "items", "t_min", "t_max")]


class DeviceSessionsStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("capacity", "slots", "items_cap", "slot_bytes", "live_bound", "sweeps", "refused", "ttl_secs", "idle_secs", "max_stored_len")]


class DeviceSessionsFileInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("version", "n", "longest_session", "items_stride", "capacity", "items_cap", "ttl_secs", "idle_secs", "saved_at_secs", "payload_bytes")]


FEEDBACK_NONE, FEEDBACK_FILLED = 0xFFFFFFFF, 0x80000000
FEEDBACK_BOOTSTRAP_MAX_ROW_CAP = 64


class FeedbackStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("capacity", "slots", "row_cap", "slot_bytes", "live_bound", "sweeps", "refused", "ttl_secs", "idle_secs",
                                          "requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")]


MAX_ARMS = 16


class Arm(C.Structure):
    """srn_arm_t: one arm of a traffic split"""
    _fields_ = [("idx", C.c_void_p), ("feedback", C.c_void_p)] + [(n, C.c_uint32) for n in ("max_items_in_session", "k", "m", "flags")]


class TrafficSplitInfo(C.Structure):
    _fields_ = [("n_arms", C.c_uint32), ("max_how_many", C.c_uint32), ("seed", C.c_uint64), ("max_batch", C.c_uint64), ("device_bytes", C.c_uint64),
                ("thresholds", C.c_uint64 * MAX_ARMS), ("served", C.c_uint64 * MAX_ARMS), ("calls", C.c_uint64), ("shortcut_calls", C.c_uint64)]


class HarvestStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("capacity", "items_cap", "min_len", "stored", "stored_items", "lost", "skipped_short", "from_return", "from_rebuild", "cleared")]


class ResultCacheStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rows", "ways", "bytes")] + [(n, C.c_uint32) for n in ("max_len", "k", "m", "how_many", "flags", "reserved")] + \
               [(n, C.c_uint64) for n in ("lookups", "hits", "inserts", "evictions", "bypassed_calls", "clears")]


class Limits(C.Structure):
    _fields_ = [("max_how_many", C.c_uint32), ("max_session_len", C.c_uint32), ("max_k", C.c_uint32), ("reserved", C.c_uint32)]


# every symbol include/serenade_hip.h and include/serenade_hip_internal.h (the srn_debug_* aids) declare: (restype, argtypes)
_vp, _sz, _u64, _i = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int
SYMBOLS = {
    "srn_sessions_from_tsv": (_i, [C.c_char_p, C.POINTER(_vp)]),
    "srn_sessions_view": (_i, [_vp, C.POINTER(SessionsView)]),
    "srn_sessions_length_quantile": (_i, [_vp, C.c_double, C.POINTER(_u64)]),
    "srn_sessions_free": (None, [_vp]),
    "srn_sessions_from_tsv_gpu": (_i, [C.c_char_p, _i, C.POINTER(_vp)]),
    "srn_sessions_from_events": (_i, [_vp, _vp, _vp, _sz, C.c_uint, _i, _vp, C.POINTER(_vp)]),
    "srn_sessions_load_info": (_i, [_vp, C.POINTER(LoadInfo)]),
    "srn_events_from_tsv_gpu": (_i, [C.c_char_p, _i, C.POINTER(_vp)]),
    "srn_events_view": (_i, [_vp, C.POINTER(EventsView)]),
    "srn_events_free": (None, [_vp]),
    "srn_events_split": (_i, [_vp, _vp, _vp, _sz, C.c_uint, C.POINTER(Split), _i, _vp, _vp, _vp, C.POINTER(SplitInfo)]),
    "srn_events_take": (_i, [_vp, _vp, _sz, C.c_uint8, _vp, _vp, _vp, C.c_uint, _vp, _vp, _vp, _i, _vp]),
    "srn_index_new_from_csv_gpu": (_i, [C.c_char_p, _sz, C.c_double, _sz, _i, C.POINTER(_vp)]),
    "srn_index_build": (_i, [C.POINTER(SessionsView), _sz, _sz, C.c_double, _i, C.POINTER(_vp)]),
    "srn_index_new_from_avro": (_i, [C.c_char_p, _i, C.POINTER(_vp)]),
    "srn_index_build_gpu": (_i, [C.POINTER(SessionsView), _sz, _sz, C.c_double, _i, C.POINTER(_vp)]),
    "srn_index_from_events_device": (_i, [_vp, _vp, _vp, _sz, C.c_uint, _sz, C.c_double, _sz, _i, _vp, C.POINTER(_vp)]),
    "srn_index_host_state": (_i, [_vp, C.POINTER(IndexHostState)]),
    "srn_index_materialize": (_i, [_vp]),
    "srn_index_new_from_csv": (_i, [C.c_char_p, _sz, C.c_double, _sz, _i, C.POINTER(_vp)]),
    "srn_index_save": (_i, [_vp, C.c_char_p]),
    "srn_index_load": (_i, [C.c_char_p, _i, C.POINTER(_vp)]),
    "srn_index_set_attributes": (_i, [_vp, _vp, _vp, _sz]),
    "srn_index_set_fallback": (_i, [_vp, _vp, _sz]),
    "srn_index_set_fallback_popular": (_i, [_vp, _sz]),
    "srn_index_fallback": (_i, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "srn_index_clear_fallback": (_i, [_vp]),
    "srn_index_info": (_i, [_vp, C.POINTER(IndexInfo)]),
    "srn_index_postings": (_i, [_vp, _u64, _vp, _sz, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "srn_index_items_for_session": (_i, [_vp, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    "srn_index_find_attributes": (_i, [_vp, _u64, C.POINTER(C.c_uint8)]),
    "srn_index_session_recency": (_i, [_vp, _vp, _sz]),
    "srn_index_serve_start": (_i, [_vp, _sz, _sz, _sz, C.c_int, C.c_uint, C.c_uint, C.c_uint]),
    "srn_index_serve_stop": (_i, [_vp]),
    "srn_index_serve_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "srn_index_result_cache_enable": (_i, [_vp, _sz, _sz, _sz, _sz, _sz, C.c_uint]),
    "srn_index_result_cache_disable": (_i, [_vp]),
    "srn_index_result_cache_clear": (_i, [_vp]),
    "srn_index_result_cache_stats": (_i, [_vp, C.POINTER(ResultCacheStats)]),
    "srn_find_neighbors": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, C.POINTER(_sz)]),
    "srn_index_free": (None, [_vp]),
    "srn_predict": (_i, [_vp, _vp, _sz, _sz, _sz, _sz, _i, _vp, _vp, C.POINTER(_sz)]),
    "srn_predict_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "srn_predict_batch": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp]),
    "srn_batcher_create": (_i, [_vp, _sz, C.c_uint, _sz, _sz, _sz, _i, C.POINTER(_vp)]),
    "srn_batcher_predict": (_i, [_vp, _vp, _sz, _vp, _vp, C.POINTER(_sz)]),
    "srn_batcher_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "srn_batcher_free": (None, [_vp]),
    "srn_batcher_how_many": (_i, [_vp, C.POINTER(_sz)]),
    "srn_session_key": (_i, [C.c_char_p, _sz, C.POINTER(_u64), C.POINTER(_u64)]),
    "srn_session_store_create": (_i, [_u64, _u64, C.POINTER(_vp)]),
    "srn_session_store_free": (None, [_vp]),
    "srn_session_store_get": (_i, [_vp, _u64, _u64, _u64, _vp, _sz, C.POINTER(_sz)]),
    "srn_session_store_update": (_i, [_vp, _u64, _u64, _u64, _vp, _sz]),
    "srn_session_store_sweep": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "srn_recommend": (_i, [_vp, _vp, C.c_char_p, _sz, _u64, _i, _sz, _u64, _vp, _vp, C.POINTER(_sz)]),
    "srn_predict_batch_device": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp]),
    "srn_predict_batch_device_excl": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp]),
    "srn_predict_batch_excl": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp]),
    "srn_debug_exclude_filter": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "srn_debug_fill": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, C.c_uint, _vp]),
    "srn_debug_class_counts": (_i, [_vp, _sz, _vp, _i]),
    "srn_debug_merge_pair": (_i, [_vp, _vp, _sz, _i]),
    "srn_predict_batch_debug": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "srn_index_reserve": (_i, [_vp, _sz, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "srn_last_kernel_ms": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "srn_index_build_shard": (_i, [C.POINTER(SessionsView), _sz, _sz, C.c_double, C.c_uint32, C.c_uint32, _i, C.POINTER(_vp)]),
    "srn_index_shard": (_i, [_vp, C.c_uint32, C.c_uint32, _i, C.POINTER(_vp)]),
    "srn_index_build_shard_gpu": (_i, [C.POINTER(SessionsView), _sz, _sz, C.c_double, C.c_uint32, C.c_uint32, _i, C.POINTER(_vp)]),
    "srn_index_load_shard": (_i, [C.c_char_p, C.c_uint32, C.c_uint32, _i, C.POINTER(_vp)]),
    "srn_shard_group_unique_id": (_i, [_vp, _sz]),
    "srn_shard_group_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "srn_shard_group_create_with_comm": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "srn_shard_group_create_local": (_i, [C.POINTER(_vp), _i, C.POINTER(_vp)]),
    "srn_shard_group_predict_batch": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp]),
    "srn_shard_group_stats": (_i, [_vp, _vp]),
    "srn_shard_group_set_overlap": (_i, [_vp, _i]),
    "srn_shard_group_wait": (_i, [_vp, _u64]),
    "srn_shard_group_set_postings": (_i, [_vp, _vp]),
    "srn_debug_shard_group_times": (_i, [_vp, _vp]),
    "srn_index_postings_view": (_i, [_vp, _i, C.POINTER(_vp)]),
    "srn_shard_group_free": (None, [_vp]),
    "srn_kernel_timing": (_i, [_vp, C.c_int]),
    "srn_kernel_times": (_i, [_vp, C.c_uint32, _vp, _vp, C.POINTER(C.c_uint32)]),
    "srn_kernel_times_detail": (_i, [_vp, C.c_uint32, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint32)]),
    "srn_debug_phase_cycles": (_i, [_vp, _i, _vp]),
    "srn_debug_reload_knobs": (None, []),
    "srn_debug_last_mid_count": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "srn_debug_last_dedup_count": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "srn_debug_last_light_count": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "srn_debug_serve_stamps": (_i, [_vp, _vp]),
    "srn_debug_serve_lane_counts": (_i, [_vp, C.c_uint, _vp, _sz, C.POINTER(_sz)]),
    "srn_debug_shard_nb_positions_stride": (C.c_uint32, [_sz, _sz]),
    "srn_debug_last_big_count": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "srn_debug_geometry": (_i, [_vp, _sz, _sz, _sz, C.c_uint, _vp]),
    "srn_debug_prep_records": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, C.POINTER(_sz)]),
    "srn_debug_sback_launches": (_i, [_vp, C.POINTER(_u64)]),
    "srn_last_path_counts": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "srn_eval_set_create": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(_vp)]),
    "srn_eval_set_from_tsv": (_i, [_vp, C.c_char_p, C.c_char_p, C.POINTER(_vp)]),
    "srn_eval_set_from_events": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, C.c_uint, _vp, C.POINTER(_vp)]),
    "srn_evaluate": (_i, [_vp, C.POINTER(EvalTrial), _sz, C.POINTER(EvalResult), _vp]),
    "srn_eval_set_free": (None, [_vp]),
    "srn_evaluate_bootstrap": (_i, [_vp, C.POINTER(EvalTrial), _sz, C.POINTER(Bootstrap), C.POINTER(EvalResult), _vp, _vp]),
    "srn_bootstrap_weights": (_i, [_u64, C.c_uint32, _u64, _sz, _vp]),
    "srn_debug_eval_terms": (_i, [_vp, C.POINTER(EvalTrial), _vp, _sz, C.POINTER(_sz), C.POINTER(EvalResult)]),
    "srn_evaluate_segments": (_i, [_vp, C.POINTER(EvalTrial), _sz, C.POINTER(Segments), C.POINTER(Bootstrap), C.POINTER(EvalResult), C.POINTER(EvalSegment), _vp, _vp, _vp]),
    "srn_eval_segment_ids": (_i, [_vp, C.POINTER(Segments), _vp, _sz, C.POINTER(_sz)]),
    "srn_debug_eval_segment_ms": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "srn_device_sessions_create": (_i, [_i, _sz, _sz, _u64, _u64, C.POINTER(_vp)]),
    "srn_device_sessions_free": (None, [_vp]),
    "srn_device_sessions_get": (_i, [_vp, _u64, _u64, _u64, _vp, _sz, C.POINTER(_sz)]),
    "srn_device_sessions_update": (_i, [_vp, _u64, _u64, _u64, _vp, _sz]),
    "srn_device_sessions_sweep": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "srn_device_sessions_stats": (_i, [_vp, C.POINTER(DeviceSessionsStats)]),
    "srn_device_sessions_timing": (_i, [_vp, _i]),
    "srn_device_sessions_last_ms": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "srn_device_sessions_count": (_i, [_vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "srn_device_sessions_export_device": (_i, [_vp, _u64, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "srn_device_sessions_export": (_i, [_vp, _u64, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "srn_device_sessions_import_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp]),
    "srn_device_sessions_import": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz]),
    "srn_device_sessions_resize": (_i, [_vp, _sz, _sz, _u64]),
    "srn_device_sessions_set_max_capacity": (_i, [_vp, _sz]),
    "srn_device_sessions_growth": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "srn_device_sessions_save": (_i, [_vp, C.c_char_p, _u64]),
    "srn_device_sessions_load": (_i, [C.c_char_p, _i, _sz, _sz, _u64, _u64, C.POINTER(_vp)]),
    "srn_device_sessions_file_info": (_i, [C.c_char_p, C.POINTER(DeviceSessionsFileInfo)]),
    "srn_device_sessions_top_items": (_i, [_vp, _u64, _u64, C.c_uint32, _sz, _vp, _vp, C.POINTER(_sz)]),
    "srn_index_set_fallback_trending": (_i, [_vp, _vp, _u64, _u64, C.c_uint32, _sz, C.c_uint, C.POINTER(_sz)]),
    "srn_session_keys": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "srn_device_sessions_set_history": (_i, [_vp, _sz]),
    "srn_device_sessions_history": (_i, [_vp, C.POINTER(_sz)]),
    "srn_recommend_batch_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp]),
    "srn_recommend_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp]),
    "srn_recommend_batch_device_at": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp, _vp]),
    "srn_recommend_batch_at": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _sz, _sz, _sz, C.c_uint, _vp, _vp, _vp]),
    "srn_feedback_observe_device_at": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp, _sz, _vp, _vp]),
    "srn_feedback_observe_at": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp, _sz, _vp]),
    "srn_debug_device_sessions_last_batch": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz), _vp, _sz, _vp]),
    "srn_feedback_create": (_i, [_i, _sz, _sz, _u64, _u64, C.POINTER(_vp)]),
    "srn_feedback_free": (None, [_vp]),
    "srn_feedback_observe_device": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp, _sz, _vp, _vp]),
    "srn_feedback_observe": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp, _sz, _vp]),
    "srn_feedback_stats": (_i, [_vp, C.POINTER(FeedbackStats)]),
    "srn_feedback_histogram": (_i, [_vp, _vp, _vp, _sz]),
    "srn_feedback_reset_counters": (_i, [_vp]),
    "srn_feedback_sweep": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "srn_feedback_get": (_i, [_vp, _u64, _u64, _u64, _vp, _sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_u64)]),
    "srn_feedback_bootstrap_enable": (_i, [_vp, C.c_uint32, _u64]),
    "srn_feedback_bootstrap_disable": (_i, [_vp]),
    "srn_feedback_bootstrap_info": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(_u64)]),
    "srn_feedback_bootstrap_read": (_i, [_vp, _vp, _vp, _vp, _sz, _sz]),
    "srn_feedback_bootstrap_weights": (_i, [_u64, C.c_uint32, _vp, _vp, _sz, _vp]),
    "srn_traffic_split_create": (_i, [_i, _vp, _sz, _u64, _sz, _sz, C.POINTER(_vp)]),
    "srn_traffic_split_free": (_i, [_vp]),
    "srn_traffic_split_info": (_i, [_vp, C.POINTER(TrafficSplitInfo)]),
    "srn_traffic_split_set_weights": (_i, [_vp, _vp, _sz]),
    "srn_traffic_split_arms": (_i, [_u64, _vp, _sz, _vp, _vp, _sz, _vp]),
    "srn_traffic_split_timing": (_i, [_vp, _i]),
    "srn_traffic_split_last_ms": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "srn_recommend_batch_split_device": (_i, [_vp, C.POINTER(Arm), _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _vp]),
    "srn_recommend_batch_split": (_i, [_vp, C.POINTER(Arm), _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "srn_harvest_create": (_i, [_i, _sz, _sz, C.c_uint32, C.POINTER(_vp)]),
    "srn_harvest_free": (_i, [_vp]),
    "srn_device_sessions_set_harvest": (_i, [_vp, _vp]),
    "srn_harvest_stats": (_i, [_vp, C.POINTER(HarvestStats)]),
    "srn_harvest_export": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "srn_harvest_export_device": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "srn_harvest_events_device": (_i, [_vp, _u64, _sz, _vp, _vp, _vp, _vp, _vp]),
    "srn_harvest_clear": (_i, [_vp]),
    "srn_device_count": (_i, [C.POINTER(_i)]),
    "srn_limits": (None, [C.POINTER(Limits)]),
    "srn_last_error": (C.c_char_p, []),
    "srn_version": (C.c_char_p, []),
}

_lib = None


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP runtimes
    in one process each open the KFD and the second one sees no GPU, so when torch is installed we load
    ITS runtime first; libserenade_hip.so's DT_NEEDED libamdhip64.so.7 then binds to it and torch
    (device memory, streams, torch.distributed/RCCL) shares one runtime with our kernels.
    SRN_HIP_RUNTIME=system skips this and uses /opt/rocm's runtime (no torch in the process then)."""
    if os.environ.get("SRN_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.submodule_search_locations:
            p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(p):
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            # and ONE RCCL: the shard group (srn_group.hip) looks for a librccl already in the process before it loads /opt/rocm's
            r = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
            if os.path.exists(r) and os.environ.get("SRN_RCCL_LIB", "") == "":
                os.environ["SRN_RCCL_LIB"] = r
    except Exception:
        pass


def lib():
    """Load the in-tree HIP library.  Fails loudly if it is missing: there is no fallback path."""
    global _lib
    if _lib is None:
        path = os.environ.get("SRN_LIB_PATH") or _build.LIB          # (SRN_LIB_PATH: a kernel variant built by build.build_variant, experiments only)
        if not os.path.exists(path):
            raise ImportError("libserenade_hip.so is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the predict path)")
        _preload_hip_runtime()
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name, None)
            if fn is None:
                if os.environ.get("SRN_LIB_PATH"):   # (an older build loaded for an A/B run: a call of what it lacks raises AttributeError there)
                    continue
                raise ImportError("%s lacks %s: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)" % (path, name))
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def reload_knobs():
    """Re-read the SRN_* test knobs from the environment (the library reads them once, at first use)."""
    lib().srn_debug_reload_knobs()


def check(rc):
    if rc != 0:
        raise SerenadeError(rc, lib().srn_last_error().decode(errors="replace"))


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def as_u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def as_u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def device_count():
    n = C.c_int()
    check(lib().srn_device_count(C.byref(n)))
    return n.value
