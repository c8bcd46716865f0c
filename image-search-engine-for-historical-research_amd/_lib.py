"""ctypes binding of libmi355_retrieval.so (include/mi355_retrieval.h).

There is no CPU fallback: if the shared library is missing or a call fails, a RuntimeError is
raised.  `load()` never builds; build with `python image-search-engine-for-historical-research_amd/build.py`
or `__graft_entry__.build()`.
"""
import contextlib
import ctypes as C
import os
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi355_retrieval.so")

MI_F32, MI_F64 = 0, 1
MI_HOST, MI_DEVICE = 0, 1
NORM_NONE, NORM_L2, NORM_L2_EPS = 0, 1, 2
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = 1, 6
MI_ERR_CAPACITY = 7
METRIC_IP, METRIC_L2 = 0, 1

c_i64p = C.POINTER(C.c_int64)
c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)


class SearchStats(C.Structure):
    _fields_ = [("searches", C.c_int64), ("queries", C.c_int64), ("overflow_batches", C.c_int64),
                ("survivors", C.c_int64), ("candidates", C.c_int64), ("gemm_ms", C.c_double),
                ("gemm_launches", C.c_int64), ("gemm_flops", C.c_double), ("gemm_bytes", C.c_double),
                ("kernel_clock_mhz", C.c_double), ("spec_retries", C.c_int64), ("inkernel_repairs", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FilterInfo(C.Structure):
    """mi_filter_info: what one mi_knn_search_filtered call did."""
    _fields_ = [("allowed", C.c_int64), ("path", C.c_int32), ("kprime", C.c_int32), ("rerun_queries", C.c_int64),
                ("cache_hit", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GroupInfo(C.Structure):
    """mi_group_info: what one mi_knn_search_grouped call did."""
    _fields_ = [("groups", C.c_int64), ("path", C.c_int32), ("kprime", C.c_int32), ("rerun_queries", C.c_int64),
                ("excluded_found", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/mi355_retrieval.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mi_last_error": (C.c_char_p, []),
    "mi_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mi_gallery_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_int,
                                    C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_gallery_create_empty": (C.c_int, [C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_gallery_append_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mi_desc_tail_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_desc_ms_accumulate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_void_p]),
    "mi_desc_ms_finish_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "mi_gallery_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "mi_gallery_remove_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    "mi_gallery_destroy": (C.c_int, [C.c_void_p]),
    "mi_gallery_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), c_i64p, c_i64p]),
    "mi_gallery_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mi_gallery_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mi_gallery_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_knn_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                C.c_void_p, C.c_void_p, c_f64p]),
    "mi_range_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_double,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_knn_search_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FilterInfo), c_f64p]),
    "mi_gallery_set_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "mi_gallery_get_groups": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_gallery_group_count": (C.c_int, [C.c_void_p, c_i64p]),
    "mi_knn_search_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GroupInfo), c_f64p]),
    "mi_gallery_create_l2": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                       C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_knn_search_l2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FilterInfo), c_f64p]),
    "mi_knn_search_l2_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mi_knn_dense64_search_l2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_refine_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mi_refine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_debug_l2_tail_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mi_knn_search_minkowski": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double,
                                          C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_knn_search_minkowski_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_range_search_minkowski": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double,
                                            C.c_double, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            c_f64p]),
    "mi_range_search_minkowski_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                                   C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_minkowski_self_range": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_graph_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_graph_build": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_graph_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mi_graph_get_neighbors": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_graph_get_entries": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_graph_destroy": (C.c_int, [C.c_void_p]),
    "mi_graph_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_graph_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "mi_forest_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_forest_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mi_forest_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32)]),
    "mi_forest_get_splits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "mi_forest_get_leaves": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "mi_forest_get_dirs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_forest_destroy": (C.c_int, [C.c_void_p]),
    "mi_forest_candidates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, c_f64p]),
    "mi_forest_candidates_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mi_forest_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, c_f64p]),
    "mi_forest_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_ivfflat_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_ivfflat_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mi_ivfflat_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_i64p]),
    "mi_ivfflat_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_ivfflat_get_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_ivfflat_get_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_ivfflat_destroy": (C.c_int, [C.c_void_p]),
    "mi_ivfflat_sync": (C.c_int, [C.c_void_p, c_i64p]),
    "mi_ivfflat_remove_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    "mi_ivfflat_probe_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "mi_ivfflat_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_hamming_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_void_p)]),
    "mi_hamming_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "mi_hamming_append_sign_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p]),
    "mi_pack_sign_bits_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "mi_hamming_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_i64p, c_i64p, c_i64p]),
    "mi_hamming_get_codes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_hamming_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, c_f64p]),
    "mi_hamming_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "mi_hamming_range_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_hamming_range_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_hamming_self_range": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        c_f64p]),
    "mi_hamming_destroy": (C.c_int, [C.c_void_p]),
    "mi_components_create": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "mi_components_reset": (C.c_int, [C.c_void_p]),
    "mi_components_add_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "mi_components_add_csr": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "mi_components_add_hamming_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]),
    "mi_components_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    "mi_components_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32)]),
    "mi_components_destroy": (C.c_int, [C.c_void_p]),
    "mi_lsh_encode_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int64, C.c_void_p]),
    "mi_lsh_encode": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
                                C.c_void_p]),
    "mi_hamming_append_lsh_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "mi_pq_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                               C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_pq_append_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "mi_pq_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "mi_pq_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "mi_pq_dtable": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_pq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, c_f64p]),
    "mi_pq_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_pq_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                             C.POINTER(C.c_int32), c_i64p, c_i64p, c_i64p]),
    "mi_pq_get_codes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_pq_get_codebooks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_pq_remove_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    "mi_pq_destroy": (C.c_int, [C.c_void_p]),
    "mi_pq_decode": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_pq_graph_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_pq_graph_build": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mi_pq_graph_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_i64p]),
    "mi_pq_graph_get_neighbors": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mi_pq_graph_get_entries": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_pq_graph_destroy": (C.c_int, [C.c_void_p]),
    "mi_pq_graph_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, c_f64p]),
    "mi_pq_graph_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "mi_pq_train": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int32, C.c_int32, C.c_int32,
                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_pq_train_timing": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mi_kmeans_train": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_kmeans_assign": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int,
                                   C.c_void_p, c_i64p]),
    "mi_kmeans_assign_workspace_bytes": (C.c_int, [C.c_int32, C.c_int64, c_i64p]),
    "mi_kmeans_assign_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mi_ivfpq_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_ivfpq_create_residual": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "mi_ivfpq_is_residual": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mi_ivfpq_residual_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int]),
    "mi_ivfpq_search_stages_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mi_ivfpq_append_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "mi_ivfpq_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "mi_ivfpq_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "mi_ivfpq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_ivfpq_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "mi_ivfpq_info": (C.c_int, [C.c_void_p, c_i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_i64p, c_i64p, c_i64p]),
    "mi_ivfpq_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_ivfpq_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "mi_ivfpq_remove_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    "mi_ivfpq_destroy": (C.c_int, [C.c_void_p]),
    "mi_knn_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "mi_knn_phase1_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "mi_kth_of_gathered_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "mi_knn_phase2_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "mi_topk_merge_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "mi_topk_merge_strided_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_aqe_partial_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                        C.c_double, C.c_void_p, C.c_void_p]),
    "mi_aqe_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "mi_aqe_combine_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "mi_aqe_finish_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "mi_aqe_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_double,
                                C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_knn_dense_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_void_p, C.c_void_p, c_f64p]),
    "mi_knn_dense64_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    "mi_rank_all": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                              C.c_void_p, c_f64p]),
    "mi_rank_prefix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int64,
                                 C.c_void_p, C.c_void_p, c_f64p]),
    "mi_rank_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int,
                                    C.c_void_p, C.c_int32, C.c_void_p]),
    "mi_kr_rerank": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                               C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "mi_diffusion_offline": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_diffusion_offline_nodes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double,
                                             C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_diffusion_set_offline": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "mi_diffusion_online": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mi_gather_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "mi_column_sum": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "mi_column_sum_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "mi_scatter_workspace_bytes": (C.c_int, [C.c_int32, c_i64p]),
    "mi_scatter_matrix_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                           C.c_void_p]),
    "mi_scatter_matrix": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "mi_gallery_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_whiten_apply": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_int32, C.c_double, C.c_int, C.c_void_p]),
    "mi_whiten_apply_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "mi_gallery_append_whitened_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64,
                                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_gallery_calibrate": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mi_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mi_search_status": (C.c_int, [C.c_void_p, C.POINTER(SearchStats), C.c_int]),
    "mi_profile_launch_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "mi_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "mi_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]),
    "mi_search_flags": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "mi_search_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi_gallery_norm_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "mi_gallery_set_image_dtype": (C.c_int, [C.c_void_p, C.c_int]),
    "mi_debug_read_cycles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mi_debug_xcc_shares": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "mi_debug_sample_source_row": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "mi_set_global_option": (C.c_int, [C.c_char_p, C.c_double]),
    "mi_get_global_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]),
    "mi_online_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_void_p)]),
    "mi_online_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_online_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mi_online_destroy": (C.c_int, [C.c_void_p]),
    "mi_debug_online_clients": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.POINTER(C.c_double)]),
    "mi_synth_fill_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
}
# the wide PQ index mirrors mi_pq entry point for entry point (uint16 codes, Ks <= 8192): the same signatures
SIGNATURES.update(("mi_pqw_" + name, SIGNATURES["mi_pq_" + name]) for name in (
    "create", "append_codes", "add", "encode", "dtable", "search", "search_device", "info", "get_codes", "get_codebooks", "decode",
    "destroy", "train"))

_lib = None
_lock = threading.Lock()


def load():
    """Loads the HIP library; raises RuntimeError (never falls back) if it is not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmi355_retrieval.so is not built (%s). Run `python __graft_entry__.py build`; "
                "this package has no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).
        # Two HIP runtimes in one process cannot both own the device, and torch tensors / streams /
        # RCCL buffers are handed to this library as raw pointers, so torch is imported first: the
        # dynamic linker then resolves our DT_NEEDED libamdhip64.so.7 to the already-loaded copy.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)        # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc):
    if rc != 0:
        msg = load().mi_last_error()
        raise RuntimeError("mi355_retrieval error %d: %s" % (rc, msg.decode() if msg else "?"))


def _strided(a):
    """(pointer, dtype code, row stride, col stride) of a 2-D float32/float64 array, in elements.
    Arrays whose strides are not whole, non-negative element multiples are copied once."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("expected a 2-D array")
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64 if a.dtype.itemsize > 4 else np.float32)
    isz = a.dtype.itemsize
    if any(s % isz or s < 0 for s in a.strides):
        a = np.ascontiguousarray(a)
    code = MI_F32 if a.dtype == np.float32 else MI_F64
    return a, code, a.strides[0] // isz, a.strides[1] // isz


def _base_pointer(a):
    """Pointer to element (0,0) plus the lowest address of the strided block."""
    return a.ctypes.data


class AllowBits(np.ndarray):
    """Packed allow words as allow_bitmap / allow_ranges return them (a uint64 ndarray).  The type is what tells packed words
    apart from an array of ids: a plain uint64 array given as `allow` is read as ids."""


def allow_bitmap(allow, n, row_offset=0, packed=False):
    """The allow bitmap of mi_knn_search_filtered for a shard of n rows starting at global id row_offset: ceil(n / 64)
    little-endian uint64 words, bit (i & 63) of word (i >> 6) allowing local row i, as an AllowBits array.  `allow` is one of
      - a bool mask [n] over the shard's rows;
      - an array or list of allowed GLOBAL ids (row_offset + local row; any integer dtype), each in the shard; an empty
        one allows no row;
      - packed words: an AllowBits array (what this function returns), or any array of ceil(n / 64) uint64 words with
        packed=True.
    Raises ValueError on ids outside the shard or a mask / word array of the wrong length."""
    n = int(n)
    nwords = (n + 63) // 64
    if packed or isinstance(allow, AllowBits):
        a = np.asarray(allow)
        if a.dtype != np.uint64 or a.shape != (nwords,):
            raise ValueError("packed bitmap of %s %s; a shard of %d rows takes %d uint64 words" % (a.dtype, a.shape, n, nwords))
        return np.ascontiguousarray(a, dtype="<u8").view(AllowBits)
    a = np.asarray(allow)
    if a.size == 0 and a.dtype != np.bool_:
        a = a.astype(np.int64)                                  # [] -> no row allowed
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError("bool mask of shape %s for a shard of %d rows" % (a.shape, n))
        mask = a
    elif np.issubdtype(a.dtype, np.integer):
        if a.dtype == np.uint64 and a.size and a.max() >= np.uint64(1 << 62):
            raise ValueError("allowed ids must lie in [%d, %d)" % (row_offset, row_offset + n))
        ids = a.reshape(-1).astype(np.int64) - int(row_offset)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise ValueError("allowed ids must lie in [%d, %d)" % (row_offset, row_offset + n))
        mask = np.zeros(n, np.bool_)
        mask[ids] = True
    else:
        raise ValueError("allow: a bool mask, an integer id array or packed AllowBits words (got %s)" % a.dtype)
    bits = np.packbits(mask, bitorder="little")
    buf = np.zeros(nwords * 8, np.uint8)
    buf[:bits.size] = bits
    return buf.view("<u8").view(AllowBits)


def allow_ranges(ranges, n, row_offset=0):
    """Allow bitmap of the union of half-open GLOBAL row ranges [(r0, r1), ...] -- the row range of each dataset of a gallery
    built by concatenating several (the reference's `--datasets A,B,...`) -- for a shard of n rows at row_offset.  The part of
    each range inside the shard is allowed; the rest is ignored.  Raises ValueError on r0 > r1 or a negative bound."""
    n = int(n)
    mask = np.zeros(n, np.bool_)
    for r0, r1 in ranges:
        r0, r1 = int(r0), int(r1)
        if r0 < 0 or r1 < r0:
            raise ValueError("bad row range (%d, %d)" % (r0, r1))
        lo, hi = max(r0 - int(row_offset), 0), min(r1 - int(row_offset), n)
        if lo < hi:
            mask[lo:hi] = True
    return allow_bitmap(mask, n)


def _allow_words(allow, n, row_offset):
    """The host words of `allow` (anything allow_bitmap takes) as the library reads them, None for allow None.  An empty bitmap
    (n = 0) becomes one zero word: the library wants a pointer all the same."""
    if allow is None:
        return None
    bits = np.asarray(allow_bitmap(allow, n, row_offset))
    return np.zeros(1, "<u8") if bits.size == 0 else bits


def _resolve_allow(allow, allow_ptr, n, row_offset):
    """The allow arguments of a host-ABI search -> (keepalive, c_void_p | None, memspace): the words of `allow` on the host
    (keepalive owns them), the device bitmap at allow_ptr, or no bitmap.  Raises ValueError when both are given."""
    if allow is not None and allow_ptr is not None:
        raise ValueError("give at most one of allow and allow_ptr")
    if allow_ptr is not None:
        return None, C.c_void_p(int(allow_ptr)), MI_DEVICE
    bits = _allow_words(allow, n, row_offset)
    return bits, None if bits is None else C.c_void_p(bits.ctypes.data), MI_HOST


def _upload_allow(bits, tdev):
    """Host allow words -> int64 tensor on the torch device `tdev` (None stays None)."""
    import torch
    return None if bits is None else torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(tdev)


def group_labels(labels):
    """Group labels as the library takes them: a contiguous int32 array [n].  Raises ValueError on labels that are no integers
    or lie outside int32 (what a label below -1 means is the library's to refuse)."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or not (np.issubdtype(lab.dtype, np.integer) or lab.dtype == np.bool_):
        raise ValueError("group labels must be a 1-D integer array")
    if lab.size and (lab.min() < -2 ** 31 or lab.max() > 2 ** 31 - 1):
        raise ValueError("group labels must fit int32")
    return np.ascontiguousarray(lab, dtype=np.int32)


MINK_L1, MINK_LINF, MINK_LP = 1, 2, 3
MINK_METRICS = {"l1": MINK_L1, "linf": MINK_LINF, "lp": MINK_LP}
MINK_MAX_K = 2048


def minkowski_args(metric, p, k):
    """The checks of a Minkowski search that need no device -> (metric code, p as the library takes it).  Raises ValueError on
    an unknown metric, on "lp" without a finite p > 0 (use "linf" for the infinite case) and on k outside [1, 2048]; p is
    ignored for "l1" and "linf"."""
    if metric not in MINK_METRICS:
        raise ValueError("metric must be 'l1', 'linf' or 'lp', got %r" % (metric,))
    if metric != "lp":
        p = 0.0
    elif p is None or not np.isfinite(float(p)) or not float(p) > 0:
        raise ValueError("metric 'lp' takes a finite p > 0 (got %r); 'linf' is the infinite case" % (p,))
    if not 1 <= int(k) <= MINK_MAX_K:
        raise ValueError("k = %d, a Minkowski search takes 1 .. %d" % (int(k), MINK_MAX_K))
    return MINK_METRICS[metric], float(p)


def minkowski_range_args(metric, p, radius):
    """The checks of a Minkowski radius search that need no device -> (metric code, p, radius as the library takes them).
    Raises ValueError on what minkowski_args refuses and on a radius that is NaN or negative (+inf is fine)."""
    code, p = minkowski_args(metric, p, 1)
    radius = float(radius)
    if not radius >= 0:
        raise ValueError("radius must be >= 0 and not NaN, got %r" % (radius,))
    return code, p, radius


def _range_capacity(nq, max_results):
    """First capacity of a range search: max_results, by default Q * 1024."""
    return int(max_results) if max_results is not None else nq * 1024


def _range_call(lock, call, nq, max_results, dtype):
    """The capacity protocol of the host range searches: `call(cap, lims, idx, val, secs)` -> rc under `lock`, once more with
    exactly lims[-1] when the first capacity was too small -> (lims int64 [nq+1], idx int64, val `dtype`, seconds)."""
    cap = _range_capacity(nq, max_results)
    lims = np.zeros(nq + 1, dtype=np.int64)
    secs = C.c_double()
    with lock:
        for attempt in range(2):
            idx = np.empty(cap, dtype=np.int64)
            val = np.empty(cap, dtype=dtype)
            rc = call(cap, lims.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p),
                      C.byref(secs))
            if rc != MI_ERR_CAPACITY or attempt == 1:
                break
            cap = int(lims[-1])
        check(rc)
    total = int(lims[-1])
    return lims, idx[:total], val[:total], secs.value


def _mink_range_call(lock, call, nq, max_results):
    """_range_call for the Minkowski radius searches, which return two value arrays: `call(cap, lims, idx, dist, dist64, secs)`
    -> (lims int64 [nq+1], idx int64, dist float32, dist64 float64, seconds)."""
    cap = _range_capacity(nq, max_results)
    lims = np.zeros(nq + 1, dtype=np.int64)
    secs = C.c_double()
    with lock:
        for attempt in range(2):
            idx = np.empty(cap, dtype=np.int64)
            dist = np.empty(cap, dtype=np.float32)
            dist64 = np.empty(cap, dtype=np.float64)
            rc = call(cap, lims.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                      dist64.ctypes.data_as(C.c_void_p), C.byref(secs))
            if rc != MI_ERR_CAPACITY or attempt == 1:
                break
            cap = int(lims[-1])
        check(rc)
    total = int(lims[-1])
    return lims, idx[:total], dist[:total], dist64[:total], secs.value


def _hbm_bytes(info, nouts):
    """The hbm_bytes property of a handle class: the last output of the library's `info`, behind `nouts` outputs not asked for."""
    def hbm_bytes(self):
        hb = C.c_int64()
        check(getattr(load(), info)(self._h, *(None,) * nouts, hb))
        return hb.value
    return property(hbm_bytes)


class _Closing:
    """`with` support and a __del__ that never raises, for a class with a close()."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle(_Closing):
    """Owner of one library handle: `_h` (None once closed), the lock that serialises the calls on it (a handle is not
    re-entrant: Flask threads in online.py) and close() through the destroy function the class names."""
    _DESTROY = None

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self._lock = threading.Lock()

    def close(self):
        """Destroys the handle; closing twice is fine.  A destroy the library refuses (mi_gallery_destroy while an online chain
        is built on the gallery) raises RuntimeError and the handle stays valid."""
        if self._h is not None and self._h.value:
            check(getattr(load(), self._DESTROY)(self._h))
            self._h = None

    def _topk(self, nq, k, dtypes, call):
        """A top-k call of the host ABI: allocates ids int64 [nq, k] and one value array [nq, k] per dtype, makes
        `call(ids, *values, seconds)` -> rc on their addresses under the lock -> (ids, *values, seconds)."""
        outs = [np.empty((nq, k), dtype=t) for t in (np.int64, *dtypes)]
        secs = C.c_double()
        with self._lock:
            check(call(*[o.ctypes.data for o in outs], C.byref(secs)))
        return (*outs, secs.value)


class Gallery(_Handle):
    """One gallery row shard resident on one MI355X (a `mi_gallery` handle)."""
    _DESTROY = "mi_gallery_destroy"

    def __init__(self, handle):
        super().__init__(handle)
        n, d = C.c_int64(), C.c_int32()
        nm, dev = C.c_int32(), C.c_int32()
        off, hb = C.c_int64(), C.c_int64()
        check(load().mi_gallery_info(self._h, n, d, nm, dev, off, hb))
        self.n, self.d, self.norm_mode, self.device = n.value, d.value, nm.value, dev.value
        self.row_offset, self.hbm_bytes = off.value, hb.value

    # ---- construction
    @classmethod
    def from_host(cls, rows, norm_mode=NORM_L2, device=0, row_offset=0):
        """rows: [N, D] float32/float64, any strides (e.g. `vecs.T` of the reference's [D, N])."""
        a, code, rs, cs = _strided(rows)
        h = C.c_void_p()
        check(load().mi_gallery_create(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs, MI_HOST,
                                       norm_mode, device, row_offset, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_device_ptr(cls, ptr, n, d, norm_mode=NORM_L2, device=0, row_offset=0, dtype=MI_F32, row_stride=None,
                        col_stride=1):
        """Device rows -> gallery, synchronous.  The ingest runs on a stream of the handle's own: the producer of `ptr` must
        have completed (torch.cuda.synchronize() / stream.synchronize()) before the call; `ptr` may be freed after it."""
        h = C.c_void_p()
        check(load().mi_gallery_create(C.c_void_p(ptr), n, d, dtype, d if row_stride is None else row_stride,
                                       col_stride, MI_DEVICE, norm_mode, device, row_offset, C.byref(h)))
        return cls(h.value)

    @classmethod
    def empty(cls, capacity, d, norm_mode=NORM_L2, device=0, row_offset=0):
        """Appendable gallery: `capacity` rows allocated, filled by append_device()."""
        h = C.c_void_p()
        check(load().mi_gallery_create_empty(capacity, d, norm_mode, device, row_offset, C.byref(h)))
        return cls(h.value)

    @classmethod
    def l2_from_host(cls, rows, device=0, row_offset=0, capacity=0, d=None):
        """Squared-L2 gallery (mi_gallery_create_l2) of rows [N, D] float32/float64, any strides, stored as given.
        capacity 0 = N; capacity > N leaves room for append() / append_device(); rows None (with d and capacity) = empty."""
        h = C.c_void_p()
        if rows is None:
            check(load().mi_gallery_create_l2(None, 0, int(d), MI_F32, int(d), 1, MI_HOST, device, row_offset, int(capacity),
                                              C.byref(h)))
        else:
            a, code, rs, cs = _strided(rows)
            check(load().mi_gallery_create_l2(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs, MI_HOST,
                                              device, row_offset, int(capacity), C.byref(h)))
        return cls(h.value)

    @classmethod
    def l2_from_device_ptr(cls, ptr, n, d, device=0, row_offset=0, capacity=0, dtype=MI_F32, row_stride=None, col_stride=1):
        """Device rows -> squared-L2 gallery, synchronous; the producer of `ptr` must have completed (see from_device_ptr)."""
        h = C.c_void_p()
        check(load().mi_gallery_create_l2(C.c_void_p(ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride,
                                          MI_DEVICE, device, row_offset, int(capacity), C.byref(h)))
        return cls(h.value)

    def append_device(self, rows_ptr, m, stream=None):
        """rows_ptr: device pointer to [m, d] float32 (C order)."""
        with self._lock:
            check(load().mi_gallery_append_device(self._h, C.c_void_p(rows_ptr), m, C.c_void_p(stream)))
            self.n += m

    def append_whitened_device(self, x_ptr, m, d, mean_ptr, p_ptr, dtype=MI_F32, row_stride=None, col_stride=1, stream=None):
        """m device rows [m, d] (strided; f32 | f64) -> P[:self.d] (x - mean), normalised by the gallery's own mode, appended.
        mean_ptr f64 [d], p_ptr f64 row-major [>= self.d, d], both on the device.  Synchronises `stream`."""
        with self._lock:
            check(load().mi_gallery_append_whitened_device(self._h, C.c_void_p(x_ptr), m, d, dtype,
                                                           d if row_stride is None else row_stride, col_stride,
                                                           C.c_void_p(mean_ptr), C.c_void_p(p_ptr), C.c_void_p(stream)))
            self.n += m

    def append(self, rows):
        """rows: [m, D] float32/float64 host array, any strides -- e.g. a column block `vecs[:, a:b].T` of the
        reference's [D, N] layout, which moves as one 2-D copy (no host transpose, no float64 promotion)."""
        a, code, rs, cs = _strided(rows)
        if a.shape[1] != self.d:
            raise ValueError("row dimension %d != gallery dimension %d" % (a.shape[1], self.d))
        with self._lock:
            check(load().mi_gallery_append(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST))
            self.n += a.shape[0]

    def remove(self, rows):
        """Removes rows in place (mi_gallery_remove_rows; faiss IndexFlat.remove_ids): `rows` is anything allow_bitmap takes
        -- a bool mask [n] over the shard's rows, an array of GLOBAL ids (duplicates are fine), or packed AllowBits words.
        The survivors keep their order and are renumbered from row_offset on.  -> kept int64 [n']: kept[j] is the old global
        id of new row j (index a list of paths with `kept - row_offset`).  Raises ValueError, before the library is called,
        on an id outside [row_offset, row_offset + n).  The image type stays; the cached sub-gallery of the filtered
        search and the offline diffusion matrix are dropped.  Refused while an OnlineChain is built on the gallery."""
        bits = allow_bitmap(rows, self.n, self.row_offset)
        gone = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), bitorder="little")[:self.n].astype(np.bool_)
        kept = np.flatnonzero(~gone).astype(np.int64) + int(self.row_offset)
        removed = C.c_int64()
        with self._lock:
            check(load().mi_gallery_remove_rows(self._h, C.c_void_p(bits.ctypes.data), MI_HOST, C.byref(removed)))
            if self.n - removed.value != kept.size:
                raise RuntimeError("mi_gallery_remove_rows removed %d rows, the bitmap names %d" % (removed.value, self.n - kept.size))
            self.n = int(kept.size)
        return kept

    @classmethod
    def from_blocks(cls, blocks, norm_mode=NORM_L2, device=0, row_offset=0, chunk_rows=131072):
        """Gallery of the concatenation `np.concatenate(blocks, axis=1).T` (src/test_rOP1m.py:136-139: [rOxford | 1M
        distractors]) WITHOUT building it on the host: every block is a [D, N_i] array (numpy, memory-mapped or a CPU
        torch tensor) and is appended in column chunks."""
        blocks = [b.numpy() if hasattr(b, "numpy") and not isinstance(b, np.ndarray) else np.asarray(b) for b in blocks]
        d = blocks[0].shape[0]
        if any(b.ndim != 2 or b.shape[0] != d for b in blocks):
            raise ValueError("blocks must be [D, N_i] arrays with one D")
        g = cls.empty(sum(b.shape[1] for b in blocks), d, norm_mode, device, row_offset)
        try:
            for b in blocks:
                for c0 in range(0, b.shape[1], chunk_rows):
                    g.append(b[:, c0:c0 + chunk_rows].T)
            if norm_mode == NORM_NONE and g.norm_bounds()[0] <= 4.0:
                g.set_image_dtype(_default_image_f16[0])      # raw rows turned out to sit inside fp16's comfortable range
        except Exception:
            g.close()
            raise
        return g

    @classmethod
    def load(cls, path, device=0):
        h = C.c_void_p()
        check(load().mi_gallery_load(os.fsencode(path), device, C.byref(h)))
        return cls(h.value)

    def save(self, path):
        check(load().mi_gallery_save(self._h, os.fsencode(path)))

    # ---- host API
    def _queries(self, q):
        """(array, dtype code, row stride, col stride) of queries [Q, d], _strided's; raises ValueError on another d."""
        a, code, rs, cs = _strided(q)
        if a.shape[1] != self.d:
            raise ValueError("query dimension %d != gallery dimension %d" % (a.shape[1], self.d))
        return a, code, rs, cs

    def search(self, queries, k):
        """-> (idx int64 [Q,k], scores float32 [Q,k], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        return self._topk(nq, k, (np.float32,), lambda idx, sc, secs: load().mi_knn_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, idx, sc, secs))

    def search_filtered(self, queries, k, allow=None, allow_ptr=None):
        """Exact top-k over the rows `allow` admits (anything allow_bitmap takes: bool mask, global ids, AllowBits words) or,
        with allow_ptr, over a device bitmap of ceil(n / 64) uint64 words -> (idx int64 [Q,k], scores float32 [Q,k], seconds,
        info dict: allowed, path, kprime, rerun_queries, cache_hit).  Fewer than k allowed rows: trailing ids -1, scores
        -inf.  Ties go to the lower id; every score is the one `search` gives that row."""
        if (allow is None) == (allow_ptr is None):
            raise ValueError("give exactly one of allow and allow_ptr")
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        bits, bits_p, memspace = _resolve_allow(allow, allow_ptr, self.n, self.row_offset)
        info = FilterInfo()
        idx, sc, secs = self._topk(nq, k, (np.float32,), lambda idx, sc, secs: load().mi_knn_search_filtered(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, int(k), bits_p, memspace, idx, sc, C.byref(info), secs))
        return idx, sc, secs, info.as_dict()

    def set_groups(self, labels):
        """One int32 label per row of the shard (mi_gallery_set_groups): labels >= 0 name a group and need not be dense, -1 makes
        the row a group of its own; None clears the groups.  append(), append_device() and remove() drop the labels: set them
        again before the next search_grouped.  Raises ValueError, before the library is called, on labels that are no integers
        or do not fit int32."""
        if labels is None:
            with self._lock:
                check(load().mi_gallery_set_groups(self._h, None, 0, MI_HOST))
            return
        lab = group_labels(labels)
        with self._lock:
            check(load().mi_gallery_set_groups(self._h, C.c_void_p(lab.ctypes.data), lab.size, MI_HOST))

    def groups(self):
        """-> the labels as given, int32 [n]."""
        out = np.empty(self.n, dtype=np.int32)
        with self._lock:
            check(load().mi_gallery_get_groups(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def group_count(self):
        """-> the number of groups, every row labelled -1 counting once."""
        out = C.c_int64()
        with self._lock:
            check(load().mi_gallery_group_count(self._h, C.byref(out)))
        return out.value

    def search_grouped(self, queries, k, exclude=None, return_labels=False, return_info=False):
        """Exact grouped top-k (mi_knn_search_grouped): search()'s ranking of every row walked from the top, one row per group
        -- the group's best, the lowest id among equal scores --, k groups per query, ordered by (that row's score desc, its id
        asc).  exclude: None, one label, or one label per query: rows of that label are skipped (-1 or a label no row carries
        skips nothing).  -> (idx int64 [Q,k], scores float32 [Q,k], seconds), then labels int32 [Q,k] (the caller's labels, -1
        for a singleton row) with return_labels and the info dict (groups, path, kprime, rerun_queries, excluded_found) with
        return_info.  Fewer than k eligible groups: trailing ids -1, scores -inf, labels -1.  Every score is the one `search`
        gives that row."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        ex = None
        if exclude is not None:
            ex = group_labels(np.broadcast_to(np.asarray(exclude), (nq,)) if np.ndim(exclude) == 0 else exclude)
            if ex.size != nq:
                raise ValueError("exclude holds %d labels for %d queries" % (ex.size, nq))
        lab = np.empty((nq, int(k)), dtype=np.int32)
        info = GroupInfo()
        idx, sc, secs = self._topk(nq, k, (np.float32,), lambda idx, sc, secs: load().mi_knn_search_grouped(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, int(k), None if ex is None else C.c_void_p(ex.ctypes.data),
            idx, sc, C.c_void_p(lab.ctypes.data), C.byref(info), secs))
        return (idx, sc, secs) + ((lab,) if return_labels else ()) + ((info.as_dict(),) if return_info else ())

    def search_l2(self, queries, k, allow=None):
        """Exact squared-L2 top-k of a gallery built by l2_from_host -> (ids int64 [Q,k], dist float32 [Q,k], dist64 float64
        [Q,k], info dict, seconds): distances ascending, ties to the lower id, fewer than k rows -> ids -1, distances +inf.
        allow: anything allow_bitmap takes (bool mask, global ids, AllowBits words) restricts the search to those rows."""
        a, code, rs, cs = self._queries(queries)
        nq, k = a.shape[0], int(k)
        bits, bits_p, memspace = _resolve_allow(allow, None, self.n, self.row_offset)
        info = FilterInfo()
        idx, dist, dist64, secs = self._topk(nq, k, (np.float32, np.float64), lambda idx, dist, dist64, secs: load().mi_knn_search_l2(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, bits_p, memspace, idx, dist, dist64, C.byref(info), secs))
        return idx, dist, dist64, info.as_dict(), secs

    def dense64_search_l2(self, queries, k):
        """Every direct-form float64 distance of the gallery + exact top-k (no threshold logic): the independent checker of
        search_l2.  -> (ids int64 [Q,k], dist float32 [Q,k], dist64 float64 [Q,k], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq, k = a.shape[0], int(k)
        return self._topk(nq, k, (np.float32, np.float64), lambda idx, dist, dist64, secs: load().mi_knn_dense64_search_l2(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, idx, dist, dist64, secs))

    def search_l2_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, dist64_ptr=None, stream=None):
        check(load().mi_knn_search_l2_device(self._h, C.c_void_p(q_ptr), nq, k, C.c_void_p(idx_ptr), C.c_void_p(dist_ptr),
                                             C.c_void_p(dist64_ptr), C.c_void_p(stream)))

    def refine(self, queries, cand, k):
        """Exact re-ranking of a shortlist on this gallery's stored rows (mi_refine; faiss IndexRefineFlat): cand integer [Q, kc]
        of GLOBAL ids from any index over the same rows, any order, repeats allowed, ids outside the shard (-1 ...) = padding ->
        (ids int64 [Q,k], val float32 [Q,k], val64 float64 [Q,k], seconds): the best k distinct candidates by (value, id asc).
        An L2 gallery gives direct-form squared distances ascending (the bits of search_l2), any other gallery inner products
        against the stored row descending, the query used as given.  Fewer than k distinct candidates: ids -1, values +inf /
        -inf.  1 <= kc <= 8192, 1 <= k <= kc."""
        a, code, rs, cs = self._queries(queries)
        c = np.asarray(cand)
        if c.ndim != 2 or c.shape[0] != a.shape[0] or c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("cand must be an integer array [Q = %d, kc] (got %s %s)" % (a.shape[0], c.dtype, c.shape))
        c = np.ascontiguousarray(c, dtype=np.int64)
        nq, kc, k = a.shape[0], c.shape[1], int(k)
        return self._topk(nq, k, (np.float32, np.float64), lambda idx, val, val64, secs: load().mi_refine(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, C.c_void_p(c.ctypes.data), kc, kc, k, idx, val, val64, secs))

    def refine_device(self, q_ptr, nq, cand_ptr, kc, k, idx_ptr, val_ptr=None, val64_ptr=None, stream=None, cand_stride=None):
        """mi_refine_device: q_ptr packed float32 [nq][d], cand_ptr int64 [nq][cand_stride or kc] on the device; enqueued on
        `stream`, no synchronisation."""
        check(load().mi_refine_device(self._h, C.c_void_p(q_ptr), int(nq), C.c_void_p(cand_ptr), int(kc),
                                      int(kc if cand_stride is None else cand_stride), int(k), C.c_void_p(idx_ptr),
                                      C.c_void_p(val_ptr), C.c_void_p(val64_ptr), C.c_void_p(stream)))

    def search_minkowski(self, queries, k, metric="l1", p=None, allow=None):
        """Exact Minkowski top-k on this gallery's stored rows (mi_knn_search_minkowski; faiss IndexFlat with METRIC_L1 /
        METRIC_Linf / METRIC_Lp): metric "l1" (sum |q - g|), "linf" (max |q - g|) or "lp" with p > 0 (sum |q - g| ** p, NOT
        raised to 1 / p), in float64 over the stored f32 row -> (ids int64 [Q,k], dist float32 [Q,k], dist64 float64 [Q,k],
        seconds): values ascending, ties to the lower id, fewer than k admitted rows -> ids -1, values +inf.  The query is used
        as given.  allow: anything allow_bitmap takes.  Raises ValueError, before the library is called, on an unknown metric,
        a p that is not finite and > 0, or k outside [1, 2048]."""
        code, p = minkowski_args(metric, p, k)
        a, dt, rs, cs = self._queries(queries)
        nq, k = a.shape[0], int(k)
        bits, bits_p, memspace = _resolve_allow(allow, None, self.n, self.row_offset)
        return self._topk(nq, k, (np.float32, np.float64), lambda idx, dist, dist64, secs: load().mi_knn_search_minkowski(
            self._h, C.c_void_p(_base_pointer(a)), nq, dt, rs, cs, code, p, k, bits_p, memspace, idx, dist, dist64, secs))

    def search_minkowski_device(self, q_ptr, nq, k, idx_ptr, metric="l1", p=None, allow_ptr=None, dist_ptr=None, dist64_ptr=None,
                                stream=None):
        """mi_knn_search_minkowski_device: q_ptr packed float32 [nq][d], allow_ptr None or a device bitmap of ceil(n / 64) uint64
        words; enqueued on `stream`, no synchronisation."""
        code, p = minkowski_args(metric, p, k)
        check(load().mi_knn_search_minkowski_device(self._h, C.c_void_p(q_ptr), int(nq), code, p, int(k), C.c_void_p(allow_ptr),
                                                    C.c_void_p(idx_ptr), C.c_void_p(dist_ptr), C.c_void_p(dist64_ptr),
                                                    C.c_void_p(stream)))

    def range_search_minkowski(self, queries, radius, metric="l1", p=None, allow=None, max_results=None):
        """Exact Minkowski radius search on this gallery's stored rows (mi_range_search_minkowski; faiss IndexFlat.range_search):
        every admitted row whose value -- search_minkowski's for that pair, bit for bit -- is <= radius (inclusive, float64) ->
        (lims int64 [Q+1], ids int64 [lims[-1]], dist float32, dist64 float64, seconds).  The hits of query i are
        ids/dist/dist64[lims[i]:lims[i+1]], ordered by (value asc, id asc); a query has 0 .. n of them.  For "lp" the radius
        applies to sum |q - g| ** p, NOT to its 1 / p-th power (a Euclidean radius r is metric="lp", p=2, radius=r * r).  allow:
        anything allow_bitmap takes.  The first call's capacity is `max_results` (default Q * 1024); if the hits do not fit, the
        call is made once more with exactly lims[-1].  Raises ValueError, before the library is called, on an unknown metric, a
        p that is not finite and > 0, a NaN or negative radius or queries of another width."""
        code, p, radius = minkowski_range_args(metric, p, radius)
        a, dt, rs, cs = self._queries(queries)
        nq = a.shape[0]
        bits, bits_p, memspace = _resolve_allow(allow, None, self.n, self.row_offset)
        lib = load()
        return _mink_range_call(
            self._lock, lambda cap, lims, idx, dist, dist64, secs: lib.mi_range_search_minkowski(
                self._h, C.c_void_p(_base_pointer(a)), nq, dt, rs, cs, code, p, radius, bits_p, memspace, cap, lims, idx, dist, dist64,
                secs),
            nq, max_results)

    def range_search_minkowski_device(self, q_ptr, nq, radius, max_results, lims_ptr, idx_ptr, metric="l1", p=None, allow_ptr=None,
                                      dist_ptr=None, dist64_ptr=None, stream=None):
        """Enqueued on `stream` without synchronising (mi_range_search_minkowski_device): q_ptr packed float32 [nq][d], lims
        [nq + 1] int64, ids / dist / dist64 [max_results] on the device.  When lims[nq] > max_results nothing is written to ids /
        dist / dist64: read lims[nq]."""
        code, p, radius = minkowski_range_args(metric, p, radius)
        check(load().mi_range_search_minkowski_device(self._h, C.c_void_p(q_ptr), int(nq), code, p, radius, C.c_void_p(allow_ptr),
                                                      int(max_results), C.c_void_p(lims_ptr), C.c_void_p(idx_ptr),
                                                      C.c_void_p(dist_ptr), C.c_void_p(dist64_ptr), C.c_void_p(stream)))

    def self_range_minkowski(self, row0, nrows, radius, metric="l1", p=None, max_results=None):
        """Stored rows [row0, row0 + nrows) as queries against the rows above each of them -> (lims int64 [nrows+1], ids, dist,
        dist64, seconds): the hits of row row0 + i are the rows j > row0 + i with value <= radius, by (value asc, j asc)
        (mi_minkowski_self_range).  The query rows never leave the device.  Capacity as in range_search_minkowski."""
        code, p, radius = minkowski_range_args(metric, p, radius)
        lib = load()
        return _mink_range_call(
            self._lock, lambda cap, lims, idx, dist, dist64, secs: lib.mi_minkowski_self_range(
                self._h, int(row0), int(nrows), code, p, radius, cap, lims, idx, dist, dist64, secs),
            int(nrows), max_results)

    def range_search(self, queries, min_score, max_results=None):
        """Every row whose exact score is >= min_score (inclusive), per query ->
        (lims int64 [Q+1], idx int64 [lims[-1]], scores float32 [lims[-1]], seconds).  The hits of query i are
        idx/scores[lims[i]:lims[i+1]], ordered by (score desc, id asc).  The first call's capacity is `max_results`
        (default Q * 1024); if the hits do not fit, the call is made once more with exactly lims[-1]."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        return _range_call(
            self._lock, lambda cap, lims, idx, sc, secs: load().mi_range_search(
                self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, float(min_score), cap, lims, idx, sc, secs),
            nq, max_results, np.float32)

    def aqe_search(self, ranks, k_qe, w, k, eps=1e-6, return_qexp=False):
        """ranks [K_in, Q] int64 (any strides) -> (idx [Q,k], scores [Q,k], qexp [Q,D] f64 | None, seconds)."""
        r = np.asarray(ranks)
        if r.dtype != np.int64:
            r = r.astype(np.int64)
        if any(s % 8 or s < 0 for s in r.strides):
            r = np.ascontiguousarray(r)
        nq = r.shape[1]
        qx = np.empty((nq, self.d), dtype=np.float64) if return_qexp else None
        idx, sc, secs = self._topk(nq, k, (np.float32,), lambda idx, sc, secs: load().mi_aqe_search(
            self._h, r.ctypes.data_as(C.c_void_p), r.strides[0] // 8, r.strides[1] // 8, nq, k_qe, float(w), float(eps), k, idx, sc,
            qx.ctypes.data_as(C.c_void_p) if return_qexp else None, secs))
        return idx, sc, qx, secs

    def dense64_search(self, queries, k):
        """Every score of the gallery in float64 + exact top-k (no threshold logic): the independent checker of the filtered
        search.  -> (idx int64 [Q,k], scores float32 [Q,k], scores float64 [Q,k], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        return self._topk(nq, k, (np.float32, np.float64), lambda idx, sc, sc64, secs: load().mi_knn_dense64_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, idx, sc, sc64, secs))

    def dense_search(self, queries, k):
        """Exact f32 inner-product top-k for large k (k <= 4096): -> (idx [Q,k], scores [Q,k], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        return self._topk(nq, k, (np.float32,), lambda idx, sc, secs: load().mi_knn_dense_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, idx, sc, secs))

    def rank_all(self, queries, query_norm=-1, return_scores=False):
        """Full-length ranking: -> (idx int64 [Q,N][, scores float32 [Q,N]], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq = a.shape[0]
        idx = np.empty((nq, self.n), dtype=np.int64)
        sc = np.empty((nq, self.n), dtype=np.float32) if return_scores else None
        secs = C.c_double()
        with self._lock:
            check(load().mi_rank_all(self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, query_norm,
                                     idx.ctypes.data_as(C.c_void_p),
                                     sc.ctypes.data_as(C.c_void_p) if return_scores else None, C.byref(secs)))
        return (idx, sc, secs.value) if return_scores else (idx, secs.value)

    def rank_prefix(self, queries, keep, query_norm=-1, return_scores=False):
        """The first `keep` columns of the full-length ranking: -> (idx int64 [Q,keep][, scores float32 [Q,keep]], seconds)."""
        a, code, rs, cs = self._queries(queries)
        nq, keep = a.shape[0], int(keep)
        idx = np.empty((nq, keep), dtype=np.int64)
        sc = np.empty((nq, keep), dtype=np.float32) if return_scores else None
        secs = C.c_double()
        with self._lock:
            check(load().mi_rank_prefix(self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, query_norm, keep,
                                        idx.ctypes.data_as(C.c_void_p),
                                        sc.ctypes.data_as(C.c_void_p) if return_scores else None, C.byref(secs)))
        return (idx, sc, secs.value) if return_scores else (idx, secs.value)

    def rank_positions(self, queries, row_ids, query_norm=-1):
        """Zero-based positions of the listed rows in every query's full ranking (score desc, idx asc), counted on the
        device.  row_ids int64 [Q, m] of global ids, -1 = padding -> position -1.  Returns int64 [Q, m]."""
        a, code, rs, cs = self._queries(queries)
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        if ids.ndim != 2 or ids.shape[0] != a.shape[0]:
            raise ValueError("row_ids must be [Q, m]")
        out = np.empty(ids.shape, dtype=np.int64)
        with self._lock:
            check(load().mi_rank_positions(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, query_norm,
                                           ids.ctypes.data_as(C.c_void_p), ids.shape[1], out.ctypes.data_as(C.c_void_p)))
        return out

    def diffusion_offline(self, n_trunc, kd, alpha=0.99, gamma=3, maxiter=20, tol=1e-6, return_sims=False):
        """-> (ids int64 [N,n_trunc], vals float32 [N,n_trunc][, knn sims float32 [N,n_trunc]])."""
        ids = np.empty((self.n, n_trunc), dtype=np.int64)
        vals = np.empty((self.n, n_trunc), dtype=np.float32)
        sims = np.empty((self.n, n_trunc), dtype=np.float32) if return_sims else None
        with self._lock:
            check(load().mi_diffusion_offline(self._h, n_trunc, kd, float(alpha), gamma, maxiter, float(tol),
                                              ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p),
                                              sims.ctypes.data_as(C.c_void_p) if return_sims else None))
        return (ids, vals, sims) if return_sims else (ids, vals)

    def diffusion_offline_nodes(self, n_trunc, kd, node0, node1, alpha=0.99, gamma=3, maxiter=20, tol=1e-6,
                                return_sims=False):
        """The offline rows of the nodes [node0, node1) only: -> (ids int64 [N,n_trunc], vals float32 [node1-node0,n_trunc]
        [, knn sims float32 [N,n_trunc]])."""
        ids = np.empty((self.n, n_trunc), dtype=np.int64)
        vals = np.empty((max(0, node1 - node0), n_trunc), dtype=np.float32)
        sims = np.empty((self.n, n_trunc), dtype=np.float32) if return_sims else None
        with self._lock:
            check(load().mi_diffusion_offline_nodes(self._h, n_trunc, kd, float(alpha), gamma, maxiter, float(tol),
                                                    int(node0), int(node1), ids.ctypes.data_as(C.c_void_p),
                                                    vals.ctypes.data_as(C.c_void_p),
                                                    sims.ctypes.data_as(C.c_void_p) if return_sims else None))
        return (ids, vals, sims) if return_sims else (ids, vals)

    def diffusion_set_offline(self, ids, vals):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.float32)
        with self._lock:
            check(load().mi_diffusion_set_offline(self._h, ids.ctypes.data_as(C.c_void_p),
                                                  vals.ctypes.data_as(C.c_void_p), ids.shape[1]))

    def diffusion_online(self, queries, k_query=3, gamma=3, trunc=2000):
        """-> (ranks int64 [Q,trunc], scores float32 [Q,trunc])."""
        a, code, rs, cs = _strided(queries)
        nq = a.shape[0]
        ranks = np.empty((nq, trunc), dtype=np.int64)
        sc = np.empty((nq, trunc), dtype=np.float32)
        with self._lock:
            check(load().mi_diffusion_online(self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k_query, gamma,
                                             trunc, ranks.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)))
        return ranks, sc

    def gather_weighted(self, ranks, weights):
        """ranks int64 [k, Q] (global ids), weights [k] -> float64 [Q, D] = sum_j weights[j] * row(ranks[j, q])."""
        r = np.ascontiguousarray(ranks, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        out = np.empty((r.shape[1], self.d), dtype=np.float64)
        with self._lock:
            check(load().mi_gather_weighted(self._h, r.ctypes.data_as(C.c_void_p), r.strides[0] // 8, r.strides[1] // 8,
                                            r.shape[1], r.shape[0], w.ctypes.data_as(C.c_void_p),
                                            out.ctypes.data_as(C.c_void_p)))
        return out

    def get_rows(self, row0, nrows):
        out = np.empty((nrows, self.d), dtype=np.float32)
        check(load().mi_gallery_get_rows(self._h, row0, nrows, out.ctypes.data_as(C.c_void_p)))
        return out

    def scatter(self, centre=None):
        """float64 [d, d] scatter matrix sum_n (g_n - centre)(g_n - centre)^T of the stored (normalised) rows; centre None = 0."""
        out = np.empty((self.d, self.d), dtype=np.float64)
        c = None if centre is None else np.ascontiguousarray(np.asarray(centre, dtype=np.float64).reshape(-1))
        if c is not None and c.shape[0] != self.d:
            raise ValueError("centre has %d entries, the gallery dimension is %d" % (c.shape[0], self.d))
        check(load().mi_gallery_scatter(self._h, None if c is None else c.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- device API (raw pointers; used by bench.py and the sharded path with torch tensors)
    def search_device(self, q_ptr, nq, k, idx_ptr, score_ptr=None, score64_ptr=None, stream=None):
        check(load().mi_knn_search_device(self._h, C.c_void_p(q_ptr), nq, k, C.c_void_p(idx_ptr),
                                          C.c_void_p(score_ptr), C.c_void_p(score64_ptr), C.c_void_p(stream)))

    def phase1_device(self, q_ptr, nq, k, approx_ptr, stream=None):
        check(load().mi_knn_phase1_device(self._h, C.c_void_p(q_ptr), nq, k, C.c_void_p(approx_ptr),
                                          C.c_void_p(stream)))

    def phase2_device(self, nq, k, L_ptr, idx_ptr, score_ptr, score64_ptr, stream=None):
        check(load().mi_knn_phase2_device(self._h, nq, k, C.c_void_p(L_ptr), C.c_void_p(idx_ptr),
                                          C.c_void_p(score_ptr), C.c_void_p(score64_ptr), C.c_void_p(stream)))

    def aqe_rows_device(self, ranks_ptr, stride_j, stride_q, nq, k_qe, rows_ptr, stream=None):
        check(load().mi_aqe_rows_device(self._h, C.c_void_p(ranks_ptr), stride_j, stride_q, nq, k_qe, C.c_void_p(rows_ptr),
                                        C.c_void_p(stream)))

    def aqe_partial_device(self, ranks_ptr, stride_j, stride_q, nq, k_qe, w, sum_ptr, stream=None):
        check(load().mi_aqe_partial_device(self._h, C.c_void_p(ranks_ptr), stride_j, stride_q, nq, k_qe, float(w),
                                           C.c_void_p(sum_ptr), C.c_void_p(stream)))

    # ---- instrumentation
    def set_option(self, name, value):
        check(load().mi_set_option(self._h, name.encode(), float(value)))

    def xcc_shares(self):
        """-> (float32 [8] shares of the XCD labels, launches that have updated them; -1 = no workspace yet)."""
        w = np.empty(8, dtype=np.float32)
        n = C.c_int32()
        check(load().mi_debug_xcc_shares(self._h, w.ctypes.data_as(C.c_void_p), C.byref(n)))
        return w, n.value

    def norm_bounds(self, raise_to=None):
        """{max ||g||, max ||g_hat||, max ||g_hat - g||} of this shard; raise_to: three floats -> the bounds become
        max(own, given) (agreement across the shards of one gallery, include/mi355_retrieval.h)."""
        b = (C.c_float * 3)(*(raise_to if raise_to is not None else (0.0, 0.0, 0.0)))
        check(load().mi_gallery_norm_bounds(self._h, b, 1 if raise_to is not None else 0))
        return [float(b[0]), float(b[1]), float(b[2])]

    def set_image_dtype(self, f16):
        check(load().mi_gallery_set_image_dtype(self._h, 1 if f16 else 0))

    def join(self, stream=None):
        """Asynchronous-tail mode: make `stream` wait for the re-score + sort of every search_device call made so far."""
        check(load().mi_search_join(self._h, C.c_void_p(stream)))

    def get_option(self, name):
        v = C.c_double(0.0)
        check(load().mi_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def flags(self):
        """Synchronises and returns (then clears) the sticky device flags of the asynchronous entry points."""
        f = C.c_uint32(0)
        check(load().mi_search_flags(self._h, C.byref(f)))
        return f.value

    def calibrate(self, launches=8, stream=None):
        """Converges the tile kernel's per-XCD shares of the gallery before the first real search (mi_gallery_calibrate)."""
        check(load().mi_gallery_calibrate(self._h, launches, C.c_void_p(stream)))

    def profile(self, on=True):
        check(load().mi_profile_enable(self._h, 1 if on else 0))

    def debug_cycles(self, nseg=2048):
        out = np.zeros((nseg, 8), dtype=np.uint64)
        check(load().mi_debug_read_cycles(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def launch_ms(self, cap=65536):
        """Durations (ms) of the timed scoring launches since the last status(reset=True), in launch order."""
        out = np.zeros(cap, dtype=np.float32)
        n = C.c_int64(0)
        check(load().mi_profile_launch_ms(self._h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:min(cap, n.value)].copy()

    def status(self, reset=False):
        st = SearchStats()
        check(load().mi_search_status(self._h, C.byref(st), 1 if reset else 0))
        return st.as_dict()


def pack_bits(a01):
    """0/1 (or bool) values [*, code_len] -> packed codes uint8 [*, ceil(code_len / 8)]: bit j of a code is bit (j & 7) of byte
    (j >> 3) (np.packbits(..., bitorder='little'), faiss's convention); a code_len that is no multiple of 8 is padded with zero
    bits.  Raises ValueError on any value other than 0 / 1."""
    a = np.asarray(a01)
    if a.ndim < 1:
        raise ValueError("expected an array [*, code_len]")
    if a.dtype != np.bool_:
        if not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
            raise ValueError("binary codes must be bool or numeric 0 / 1 values (got %s)" % a.dtype)
        if a.size and not np.logical_or(a == 0, a == 1).all():
            raise ValueError("binary codes must hold only the values 0 and 1")
        a = a != 0
    return np.packbits(a, axis=-1, bitorder="little")


def unpack_bits(codes, code_len=None):
    """Inverse of pack_bits: uint8 [*, nbytes] -> uint8 0/1 [*, code_len] (default 8 * nbytes)."""
    bits = np.unpackbits(np.asarray(codes, np.uint8), axis=-1, bitorder="little")
    return bits if code_len is None else bits[..., :int(code_len)]


def pack_sign_bits_device(x_ptr, n, d, out_ptr, row_stride=None, out_row_stride=None, stream=None):
    """Device rows x [n][d] f32 -> packed sign codes [n][d / 8] uint8 on the device (bit j = x[j] > 0), enqueued on `stream`."""
    check(load().mi_pack_sign_bits_device(C.c_void_p(x_ptr), int(n), int(d), int(d if row_stride is None else row_stride),
                                          C.c_void_p(out_ptr), int(d // 8 if out_row_stride is None else out_row_stride),
                                          C.c_void_p(stream)))


def _code_rows(codes, nbytes=None):
    """uint8 [m, nbytes] with a whole-byte, non-negative row stride and contiguous rows (copied once otherwise)."""
    a = np.asarray(codes)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("packed codes must be a uint8 array [rows, nbits / 8] (see pack_bits)")
    if nbytes is not None and a.shape[1] != nbytes:
        raise ValueError("codes of %d bytes, the index holds codes of %d bytes" % (a.shape[1], nbytes))
    if a.shape[1] > 1 and a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a, max(int(a.strides[0]), a.shape[1])


REFINE_MAX_KC = 8192


GRAPH_MAX_EF, GRAPH_MAX_R, GRAPH_MAX_ENTRIES = 2048, 64, 64


def _graph_search_shape(k, ef):
    """(k, ef) of a graph search, ef defaulting to max(k, 64); raises ValueError outside 1 <= k <= ef <= 2048."""
    k = int(k)
    ef = max(k, 64) if ef is None else int(ef)
    if ef < 1 or ef > GRAPH_MAX_EF:
        raise ValueError("ef = %d: ef must be in [1, %d]" % (ef, GRAPH_MAX_EF))
    if k < 1 or k > ef:
        raise ValueError("k = %d: k must be in [1, ef = %d]" % (k, ef))
    return k, ef


def _graph_build_shape(n, R, n_entry):
    """Raises ValueError unless R is even in [2, 64], 1 <= n_entry <= 64 and n >= 2 (mi_graph_build)."""
    R, n_entry = int(R), int(n_entry)
    if R < 2 or R > GRAPH_MAX_R or R % 2:
        raise ValueError("R = %d: R must be even and in [2, %d]" % (R, GRAPH_MAX_R))
    if n_entry < 1 or n_entry > GRAPH_MAX_ENTRIES:
        raise ValueError("n_entry = %d: the number of entry rows must be in [1, %d]" % (n_entry, GRAPH_MAX_ENTRIES))
    if int(n) < 2:
        raise ValueError("a graph is built over at least two rows (the gallery holds %d)" % n)
    return R, n_entry


def _graph_table(n, table, entries):
    """(table int32 [n, R] C-contiguous, entries int32 [ne]) of GraphIndex.from_neighbors; raises ValueError on a table of another
    shape, R or ne outside [1, 64], an entry outside [0, n) or a table value below -1 or >= n."""
    t, e = np.asarray(table), np.asarray(entries)
    for name, a in (("table", t), ("entries", e)):
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("%s must be an integer array (got %s)" % (name, a.dtype))
    if t.ndim != 2 or t.shape[0] != int(n) or not 1 <= t.shape[1] <= GRAPH_MAX_R:
        raise ValueError("table of shape %s; a gallery of %d rows takes [%d, R] with R in [1, %d]" % (t.shape, n, n, GRAPH_MAX_R))
    if e.ndim != 1 or not 1 <= e.shape[0] <= GRAPH_MAX_ENTRIES:
        raise ValueError("entries of shape %s; give 1 .. %d entry rows" % (e.shape, GRAPH_MAX_ENTRIES))
    if e.min() < 0 or e.max() >= n:
        raise ValueError("entry rows must lie in [0, %d)" % n)
    if t.size and (t.min() < -1 or t.max() >= n):
        raise ValueError("table values must be -1 (padding) or lie in [0, %d)" % n)
    return np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(e, dtype=np.int32)


class _GraphBase(_Handle):
    """What GraphIndex and PQGraphIndex share: the handle of a `<_PREFIX>*` graph over an owner index (kept as the attribute
    _OWNER names, which must outlive the graph), its table and its entry rows."""
    _PREFIX = _OWNER = None
    _INFO_EXTRA = ()                   # arguments of <_PREFIX>_info behind n, R and ne

    def __init__(self, handle, owner):
        super().__init__(handle)
        setattr(self, self._OWNER, owner)
        n, R, ne = C.c_int64(), C.c_int32(), C.c_int32()
        check(self._fn("info")(self._h, n, R, ne, *self._INFO_EXTRA))
        self.n, self.R, self.n_entry = n.value, R.value, ne.value

    @classmethod
    def _fn(cls, name):
        return getattr(load(), "%s_%s" % (cls._PREFIX, name))

    @classmethod
    def build(cls, owner, R=32, n_entry=16):
        """<_PREFIX>_build: per row its R / 2 nearest rows, up to R / 2 reverse edges, then further nearest rows up to R entries;
        min(n_entry, n) evenly spaced entry rows.  Deterministic; runs on the device."""
        R, n_entry = _graph_build_shape(owner.n, R, n_entry)
        h = C.c_void_p()
        with owner._lock:
            check(cls._fn("build")(owner._h, R, n_entry, C.byref(h)))
        return cls(h.value, owner)

    @classmethod
    def from_neighbors(cls, owner, table, entries):
        """<_PREFIX>_create: table integer [n, R] of LOCAL rows (-1 = padding; self-loops and repeats are legal), entries integer
        [ne] local rows.  Bad input raises ValueError before the device is touched."""
        t, e = _graph_table(owner.n, table, entries)
        h = C.c_void_p()
        with owner._lock:
            check(cls._fn("create")(owner._h, C.c_void_p(t.ctypes.data), t.shape[1], MI_HOST, C.c_void_p(e.ctypes.data), e.shape[0],
                                    C.byref(h)))
        return cls(h.value, owner)

    @property
    def neighbors(self):
        """The table, int32 [n, R]."""
        out = np.empty((self.n, self.R), np.int32)
        with self._lock:
            check(self._fn("get_neighbors")(self._h, 0, self.n, C.c_void_p(out.ctypes.data)))
        return out

    @property
    def entries(self):
        """The entry rows, int32 [n_entry]."""
        out = np.empty(self.n_entry, np.int32)
        with self._lock:
            check(self._fn("get_entries")(self._h, C.c_void_p(out.ctypes.data)))
        return out


class GraphIndex(_GraphBase):
    """A neighbour graph over the rows of a Gallery (a `mi_graph` handle): best-first search from a set of entry
    rows, the role of the reference's HNSW matchers.  Which rows the graph reaches is approximate; the answer given graph, entry
    rows, stored rows and query is exact: values are Gallery.refine's (direct-form float64 squared distances on an L2 gallery,
    float64 inner products against the stored row on any other), the order is (value best first, id ascending).  The gallery
    must outlive the index; after gallery.append* / gallery.remove a search raises (build a new graph)."""

    _PREFIX, _OWNER, _DESTROY = "mi_graph", "gallery", "mi_graph_destroy"

    def search(self, q, k, ef=None, return_visited=False, return_values64=False):
        """-> (ids int64 [Q, k], values float32 [Q, k], seconds); ef (the size of the candidate list W) defaults to max(k, 64),
        1 <= k <= ef <= 2048.  Fewer than k rows reached: ids -1, values +inf (L2) / -inf.  return_values64: the float64 values
        in place of their float32 cast; return_visited: int32 [Q], the rows evaluated per query, appended to the tuple."""
        k, ef = _graph_search_shape(k, ef)
        a, code, rs, cs = self.gallery._queries(q)
        nq = a.shape[0]
        vis = np.empty(nq, dtype=np.int32)
        idx, val, val64, secs = self._topk(nq, k, (np.float32, np.float64), lambda idx, val, val64, secs: load().mi_graph_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, ef, idx, val, val64, C.c_void_p(vis.ctypes.data), secs))
        out = (idx, val64 if return_values64 else val, secs)
        return out + (vis,) if return_visited else out

    def search_device(self, q_ptr, nq, k, idx_ptr, ef=None, val_ptr=None, val64_ptr=None, visited_ptr=None, stream=None):
        """mi_graph_search_device: q_ptr packed float32 [nq][d] on the device; enqueued on `stream`, no synchronisation."""
        k, ef = _graph_search_shape(k, ef)
        check(load().mi_graph_search_device(self._h, C.c_void_p(q_ptr), int(nq), k, ef, C.c_void_p(idx_ptr), C.c_void_p(val_ptr),
                                            C.c_void_p(val64_ptr), C.c_void_p(visited_ptr), C.c_void_p(stream)))


FOREST_MAX_T, FOREST_MAX_L, FOREST_MAX_D, FOREST_LEAF_TARGET = 256, 24, 4096, 64


def _forest_check(n, d, T, L):
    """leaf_max = ceil(n / 2^L) of a forest of T trees with L levels of splits over n rows of d columns; raises ValueError outside
    1 <= T <= 256, 1 <= L <= 24, 2^L <= n < 2^31, d <= 4096, T * leaf_max <= 8192 (mi_forest_build's and mi_forest_create's checks)."""
    n, d, T, L = int(n), int(d), int(T), int(L)
    if T < 1 or T > FOREST_MAX_T:
        raise ValueError("T = %d: T must be in [1, %d]" % (T, FOREST_MAX_T))
    if L < 1 or L > FOREST_MAX_L:
        raise ValueError("L = %d: L must be in [1, %d]" % (L, FOREST_MAX_L))
    if n >= 2 ** 31 or d > FOREST_MAX_D:
        raise ValueError("a forest takes fewer than 2^31 rows of d <= %d columns (got %d x %d)" % (FOREST_MAX_D, n, d))
    if (1 << L) > n:
        raise ValueError("L = %d: 2^L must not exceed the %d rows of the gallery" % (L, n))
    leaf_max = -(-n // (1 << L))
    if T * leaf_max > REFINE_MAX_KC:
        raise ValueError("T * leaf_max = %d candidates per query: at most %d (more levels or fewer trees)" % (T * leaf_max, REFINE_MAX_KC))
    return leaf_max


def _forest_shape(k_hint, n, n_trees):
    """The depth ForestIndex.build picks where none is given: the smallest L >= 1 with leaf_max = ceil(n / 2^L) <= 64 and
    n_trees * leaf_max <= 8192, subject to 2^L <= n and L <= 24 -> (L, leaf_max).  Leaves of up to 64 rows keep a tree's share of the
    candidates small next to the union of all trees; the second bound is mi_refine's.  k_hint (None: no wish) is the k the caller
    will search with: a forest whose n_trees * leaf_max slots cannot hold k rows raises.  ValueError where no such L exists
    (n < 2, n_trees outside [1, 256], n beyond 64 * 2^24 rows)."""
    n, T = int(n), int(n_trees)
    if T < 1 or T > FOREST_MAX_T:
        raise ValueError("n_trees = %d: T must be in [1, %d]" % (T, FOREST_MAX_T))
    for L in range(1, FOREST_MAX_L + 1):
        if (1 << L) > n:
            break
        leaf_max = -(-n // (1 << L))
        if leaf_max <= FOREST_LEAF_TARGET and T * leaf_max <= REFINE_MAX_KC:
            if k_hint is not None and int(k_hint) > T * leaf_max:
                raise ValueError("k = %d: %d trees with leaves of %d rows give %d candidates per query" % (k_hint, T, leaf_max, T * leaf_max))
            return L, leaf_max
    raise ValueError("no depth L in [1, %d] with 2^L <= n = %d gives leaves of at most %d rows and at most %d candidates per query "
                     "for %d trees" % (FOREST_MAX_L, n, FOREST_LEAF_TARGET, REFINE_MAX_KC, T))


def forest_directions(d, T, L, seed=5):
    """Standard normal float64 [T * L, d] from numpy's seeded Generator: row t * L + l is the direction of level l of tree t."""
    d, T, L = int(d), int(T), int(L)
    if d < 1 or T < 1 or L < 1:
        raise ValueError("forest_directions: d, T and L must be >= 1 (got %d, %d, %d)" % (d, T, L))
    return np.random.default_rng(seed).standard_normal((T * L, d))


def _forest_dirs(dirs, d, T, L):
    """dirs as float64 [T * L, d] C-contiguous; raises ValueError on another shape or a value that is not finite."""
    a = np.ascontiguousarray(dirs, dtype=np.float64)
    if a.shape != (T * L, d):
        raise ValueError("dirs of shape %s; %d trees of %d levels over %d columns take [%d, %d]" % (a.shape, T, L, d, T * L, d))
    if not np.isfinite(a).all():
        raise ValueError("dirs must be finite")
    return a


def _forest_trees(n, d, dirs, splits, leaves):
    """(dirs float64 [T L, d], splits float64 [T, 2^L - 1], leaves int32 [T, n], T, L) of ForestIndex.from_trees; T and L are read
    off leaves and splits.  Raises ValueError on arrays of other shapes, a leaf value outside [0, n) and whatever _forest_check
    refuses."""
    s, lv = np.asarray(splits), np.asarray(leaves)
    if lv.dtype == np.bool_ or not np.issubdtype(lv.dtype, np.integer):
        raise ValueError("leaves must be an integer array (got %s)" % lv.dtype)
    if lv.ndim != 2 or lv.shape[1] != int(n):
        raise ValueError("leaves of shape %s; a gallery of %d rows takes [T, %d]" % (lv.shape, n, n))
    T = lv.shape[0]
    L = int(s.shape[1] + 1).bit_length() - 1 if s.ndim == 2 else 0
    if s.ndim != 2 or s.shape[0] != T or s.shape[1] != (1 << L) - 1 or not np.issubdtype(s.dtype, np.floating):
        raise ValueError("splits of shape %s %s; %d trees take float [%d, 2^L - 1]" % (s.dtype, s.shape, T, T))
    _forest_check(n, d, T, L)
    if lv.size and (lv.min() < 0 or lv.max() >= n):
        raise ValueError("leaf values must lie in [0, %d)" % n)
    return (_forest_dirs(dirs, int(d), T, L), np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(lv, dtype=np.int32), T, L)


class ForestIndex(_Handle):
    """A forest of random-projection trees over the rows of a Gallery (a `mi_forest` handle), the role of the
    reference's matching_ANNOY.  T balanced trees; every node of one level of one tree splits its rows at the median of their
    projection onto that level's direction; a query descends every tree and the rows of the T leaves it reaches are re-ranked
    exactly.  Which rows the forest reaches is approximate; the answer given directions, trees, stored rows and query is exact:
    values are Gallery.refine's, the order is (value best first, id ascending).  The gallery must outlive the index; after
    gallery.append* / gallery.remove a search raises (build a new forest).  These are this library's trees, not annoy's."""
    _DESTROY = "mi_forest_destroy"

    def __init__(self, handle, gallery):
        super().__init__(handle)
        self.gallery = gallery
        n, d, T, L, lm = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(load().mi_forest_info(self._h, n, d, T, L, lm))
        self.n, self.d, self.n_trees, self.depth, self.leaf_max = n.value, d.value, T.value, L.value, lm.value

    @classmethod
    def build(cls, gallery, n_trees=100, depth=None, seed=5, dirs=None):
        """mi_forest_build: n_trees trees of `depth` levels of splits (None: _forest_shape's choice) on the directions `dirs`
        (float [n_trees * depth, d]; None: forest_directions(d, n_trees, depth, seed)).  Deterministic; runs on the device.  Bad
        shapes raise ValueError before the device is touched."""
        T = int(n_trees)
        L = _forest_shape(None, gallery.n, T)[0] if depth is None else int(depth)
        _forest_check(gallery.n, gallery.d, T, L)
        r = forest_directions(gallery.d, T, L, seed) if dirs is None else _forest_dirs(dirs, gallery.d, T, L)
        h = C.c_void_p()
        with gallery._lock:
            check(load().mi_forest_build(gallery._h, C.c_void_p(r.ctypes.data), T, L, C.byref(h)))
        return cls(h.value, gallery)

    @classmethod
    def from_trees(cls, gallery, dirs, splits, leaves):
        """mi_forest_create: dirs float [T * L, d], splits float [T, 2^L - 1], leaves integer [T, n] of LOCAL rows (repeats are
        legal).  Bad input raises ValueError before the device is touched."""
        r, s, lv, T, L = _forest_trees(gallery.n, gallery.d, dirs, splits, leaves)
        h = C.c_void_p()
        with gallery._lock:
            check(load().mi_forest_create(gallery._h, C.c_void_p(r.ctypes.data), T, L, C.c_void_p(s.ctypes.data),
                                          C.c_void_p(lv.ctypes.data), MI_HOST, C.byref(h)))
        return cls(h.value, gallery)

    def _k(self, k):
        k = int(k)
        if k < 1 or k > self.n_trees * self.leaf_max:
            raise ValueError("k = %d: k must be in [1, T * leaf_max = %d]" % (k, self.n_trees * self.leaf_max))
        return k

    def search(self, q, k, return_values64=False):
        """-> (ids int64 [Q, k], values float32 [Q, k], seconds), 1 <= k <= n_trees * leaf_max.  Fewer than k distinct rows in the
        leaves reached: ids -1, values +inf (L2) / -inf.  return_values64: the float64 values in place of their float32 cast."""
        k = self._k(k)
        a, code, rs, cs = self.gallery._queries(q)
        nq = a.shape[0]
        idx, val, val64, secs = self._topk(nq, k, (np.float32, np.float64), lambda idx, val, val64, secs: load().mi_forest_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, idx, val, val64, secs))
        return idx, val64 if return_values64 else val, secs

    def search_device(self, q_ptr, nq, k, idx_ptr, val_ptr=None, val64_ptr=None, stream=None):
        """mi_forest_search_device: q_ptr packed float32 [nq][d] on the device; enqueued on `stream`, no synchronisation."""
        check(load().mi_forest_search_device(self._h, C.c_void_p(q_ptr), int(nq), self._k(k), C.c_void_p(idx_ptr), C.c_void_p(val_ptr),
                                             C.c_void_p(val64_ptr), C.c_void_p(stream)))

    def candidates(self, q):
        """-> int64 [Q, n_trees * leaf_max]: slot t * leaf_max + i is the i-th row (global id) of the leaf the query reaches in
        tree t, -1 behind a leaf shorter than leaf_max (mi_forest_candidates)."""
        a, code, rs, cs = self.gallery._queries(q)
        out = np.empty((a.shape[0], self.n_trees * self.leaf_max), np.int64)
        with self._lock:
            check(load().mi_forest_candidates(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs,
                                              C.c_void_p(out.ctypes.data), None))
        return out

    def splits(self):
        """The split values, float64 [n_trees, 2^depth - 1]: node (l, j) at column 2^l - 1 + j."""
        out = np.empty((self.n_trees, (1 << self.depth) - 1), np.float64)
        with self._lock:
            check(load().mi_forest_get_splits(self._h, 0, self.n_trees, C.c_void_p(out.ctypes.data)))
        return out

    def leaves(self):
        """The row permutations, int32 [n_trees, n]."""
        out = np.empty((self.n_trees, self.n), np.int32)
        with self._lock:
            check(load().mi_forest_get_leaves(self._h, 0, self.n_trees, C.c_void_p(out.ctypes.data)))
        return out

    def dirs(self):
        """The directions, float64 [n_trees * depth, d]."""
        out = np.empty((self.n_trees * self.depth, self.d), np.float64)
        with self._lock:
            check(load().mi_forest_get_dirs(self._h, C.c_void_p(out.ctypes.data)))
        return out


def refine_kc(k, k_factor, n):
    """Length of the shortlist an index search hands to Gallery.refine_device: min(k * k_factor, n, 8192), never below k."""
    k, f = int(k), int(k_factor)
    if f < 1:
        raise ValueError("k_factor = %d: the shortlist is k * k_factor ids, k_factor >= 1" % f)
    return max(k, min(k * f, int(n), REFINE_MAX_KC))


_NO_ALLOW = (None, None, MI_HOST)          # what _resolve_allow gives a search without an allow list


def _search_refined(rows, q, k, kc, allow, device, lock, search_device, stage=None, **kw):
    """The refine= path of the index searches: q float32 [Q, d] host rows, allow what _resolve_allow returned.  The index's own
    search_device(q_ptr, nq, kc, cand_ptr, stream=, allow_ptr= where there are allow words, **kw) is enqueued under `lock`
    (None: no lock) for kc ids per query; rows.refine_device follows on the same stream, and only the final k ids and exact
    values come back -> (ids int64 [Q,k], val float32 [Q,k], seconds).  An index that does not search the float32 rows as they
    are gives stage(xq, stream) -> (the device tensor its search reads as queries, {keyword: device tensor passed as pointer})."""
    import torch
    bits, _, memspace = allow
    if memspace == MI_DEVICE:
        raise ValueError("refine takes allow, not allow_ptr")
    if not isinstance(rows, Gallery):
        raise ValueError("refine must be a Gallery that holds the raw rows (got %s)" % type(rows).__name__)
    a = np.ascontiguousarray(q, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != rows.d:
        raise ValueError("refine: queries of %s columns, the rows gallery holds %d" % (a.shape[1:], rows.d))
    if rows.device != device:
        raise ValueError("refine: the rows gallery is on device %d, the index on device %d" % (rows.device, device))
    nq, k = a.shape[0], int(k)
    if nq == 0:
        return np.empty((0, k), np.int64), np.empty((0, k), np.float32), 0.0
    tdev = "cuda:%d" % device
    t0 = time.perf_counter()
    stream = torch.cuda.current_stream(tdev).cuda_stream
    xq = torch.from_numpy(a).to(tdev)
    bits_dev = _upload_allow(bits, tdev)
    cand = torch.empty((nq, kc), dtype=torch.int64, device=tdev)
    idx = torch.empty((nq, k), dtype=torch.int64, device=tdev)
    val = torch.empty((nq, k), dtype=torch.float32, device=tdev)
    q_dev, staged = (xq, {}) if stage is None else stage(xq, stream)
    kw.update((name, t.data_ptr()) for name, t in staged.items())
    if bits_dev is not None:
        kw["allow_ptr"] = bits_dev.data_ptr()
    with lock or contextlib.nullcontext():
        search_device(q_dev.data_ptr(), nq, kc, cand.data_ptr(), stream=stream, **kw)
    with rows._lock:
        rows.refine_device(xq.data_ptr(), nq, cand.data_ptr(), kc, k, idx.data_ptr(), val_ptr=val.data_ptr(), stream=stream)
        ids, vv = idx.cpu().numpy(), val.cpu().numpy()           # (synchronises with the stream the work is on)
    return ids, vv, time.perf_counter() - t0


class BinaryGallery(_Handle):
    """Binary index on one MI355X (a `mi_hamming` handle): exact Hamming top-k on packed codes, ties to the lower id."""
    _DESTROY = "mi_hamming_destroy"
    hbm_bytes = _hbm_bytes("mi_hamming_info", 5)

    def __init__(self, handle):
        super().__init__(handle)
        n, nbits, dev, off, cap, hb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        check(load().mi_hamming_info(self._h, n, nbits, dev, off, cap, hb))
        self.n, self.nbits, self.device, self.row_offset, self.capacity = n.value, nbits.value, dev.value, off.value, cap.value

    @classmethod
    def from_host(cls, codes, device=0, row_offset=0, capacity=0):
        """codes: uint8 [N, nbits / 8] (pack_bits); capacity 0 = N, larger leaves room for append()."""
        a, stride = _code_rows(codes)
        h = C.c_void_p()
        check(load().mi_hamming_create(C.c_void_p(a.ctypes.data), a.shape[0], a.shape[1] * 8, stride, MI_HOST, device,
                                       row_offset, int(capacity), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_device_ptr(cls, ptr, n, nbits, device=0, row_offset=0, capacity=0, row_stride_bytes=None):
        """Device codes [n][nbits / 8] uint8 -> index, synchronous; the producer of `ptr` must have completed."""
        h = C.c_void_p()
        check(load().mi_hamming_create(C.c_void_p(ptr), int(n), int(nbits),
                                       int(nbits) // 8 if row_stride_bytes is None else int(row_stride_bytes), MI_DEVICE, device,
                                       row_offset, int(capacity), C.byref(h)))
        return cls(h.value)

    @classmethod
    def empty(cls, capacity, nbits, device=0, row_offset=0):
        """Appendable index: `capacity` rows allocated, filled by append() / append_sign_device()."""
        h = C.c_void_p()
        check(load().mi_hamming_create(None, 0, int(nbits), int(nbits) // 8, MI_HOST, device, row_offset, int(capacity),
                                       C.byref(h)))
        return cls(h.value)

    def append(self, codes):
        a, stride = _code_rows(codes, self.nbits // 8)
        with self._lock:
            check(load().mi_hamming_append(self._h, C.c_void_p(a.ctypes.data), a.shape[0], stride, MI_HOST))
            self.n += a.shape[0]

    def append_sign_device(self, x_ptr, m, d, row_stride=None, stream=None):
        """m device rows [m][d] f32, d == nbits: their sign bits (x > 0) are appended on `stream`."""
        with self._lock:
            check(load().mi_hamming_append_sign_device(self._h, C.c_void_p(x_ptr), int(m), int(d),
                                                       int(d if row_stride is None else row_stride), C.c_void_p(stream)))
            self.n += int(m)

    def append_lsh_device(self, x_ptr, m, d, r_ptr, thr_ptr=None, dtype=MI_F32, row_stride=None, col_stride=1, stream=None):
        """m device rows of d elements: the LSH codes of their projections (x . R[j] >= t[j]; R float64 [nbits][d] and t float64
        [nbits] or None on the device) are appended on `stream` (mi_hamming_append_lsh_device)."""
        with self._lock:
            check(load().mi_hamming_append_lsh_device(self._h, C.c_void_p(x_ptr), int(m), int(d), dtype,
                                                      int(d if row_stride is None else row_stride), int(col_stride),
                                                      C.c_void_p(r_ptr), C.c_void_p(thr_ptr), C.c_void_p(stream)))
            self.n += int(m)

    def search(self, qcodes, k, allow=None, allow_ptr=None, refine=None, k_factor=1, refine_queries=None):
        """-> (ids int64 [Q,k], dist int32 [Q,k], seconds), ordered by (distance asc, id asc).  allow: anything allow_bitmap
        takes (bool mask, global ids, AllowBits words); allow_ptr: a device bitmap of ceil(n / 64) uint64 words.  Fewer than k
        admitted rows: trailing ids -1, distances INT32_MAX.
        refine=<Gallery of the raw rows> with refine_queries [Q, d] (the raw queries behind qcodes): the Hamming search takes
        refine_kc(k, k_factor, n) ids on the device, the gallery re-ranks them there (Gallery.refine) and the distances returned
        are its exact float32 values."""
        a, stride = _code_rows(qcodes, self.nbits // 8)
        nq, k = a.shape[0], int(k)
        resolved = bits, bits_p, memspace = _resolve_allow(allow, allow_ptr, self.n, self.row_offset)
        if refine is not None:
            import torch
            if refine_queries is None or np.shape(refine_queries)[0] != nq:
                raise ValueError("refine: give refine_queries [Q = %d, d], the raw queries behind the codes" % nq)
            packed = np.ascontiguousarray(a)
            return _search_refined(refine, refine_queries, k, refine_kc(k, k_factor, self.n), resolved, self.device, self._lock,
                                   self.search_device, stage=lambda xq, stream: (torch.from_numpy(packed).to(xq.device), {}))
        return self._topk(nq, k, (np.int32,), lambda idx, dist, secs: load().mi_hamming_search(
            self._h, C.c_void_p(a.ctypes.data), nq, stride, k, bits_p, memspace, idx, dist, secs))

    def search_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, allow_ptr=None, stream=None):
        check(load().mi_hamming_search_device(self._h, C.c_void_p(q_ptr), int(nq), int(k), C.c_void_p(allow_ptr),
                                              C.c_void_p(idx_ptr), C.c_void_p(dist_ptr), C.c_void_p(stream)))

    def range_search(self, qcodes, radius, allow=None, max_results=None, allow_ptr=None):
        """Every admitted row within `radius` bits (inclusive) of each query ->
        (lims int64 [Q+1], ids int64 [lims[-1]], dist int32 [lims[-1]], seconds).  The hits of query i are
        ids/dist[lims[i]:lims[i+1]], ordered by (distance asc, id asc); a query has 0 .. n of them.  allow / allow_ptr as in
        search().  The first call's capacity is `max_results` (default Q * 1024); if the hits do not fit, the call is made once
        more with exactly lims[-1]."""
        a, stride = _code_rows(qcodes, self.nbits // 8)
        bits, bits_p, memspace = _resolve_allow(allow, allow_ptr, self.n, self.row_offset)
        lib = load()
        return _range_call(
            self._lock, lambda cap, lims, idx, dist, secs: lib.mi_hamming_range_search(
                self._h, C.c_void_p(a.ctypes.data), a.shape[0], stride, int(radius), bits_p, memspace, cap, lims, idx, dist, secs),
            a.shape[0], max_results, np.int32)

    def range_search_device(self, q_ptr, nq, radius, max_results, lims_ptr, idx_ptr, dist_ptr=None, allow_ptr=None, stream=None):
        """Enqueued on `stream` without synchronising (mi_hamming_range_search_device): lims [nq + 1] int64, ids / dist
        [max_results] on the device.  When lims[nq] > max_results nothing is written to ids / dist: read lims[nq]."""
        check(load().mi_hamming_range_search_device(self._h, C.c_void_p(q_ptr), int(nq), int(radius), C.c_void_p(allow_ptr),
                                                    int(max_results), C.c_void_p(lims_ptr), C.c_void_p(idx_ptr),
                                                    C.c_void_p(dist_ptr), C.c_void_p(stream)))

    def self_range(self, row0, nrows, radius, max_results=None):
        """Stored rows [row0, row0 + nrows) as queries against the rows above each of them -> (lims int64 [nrows+1], ids, dist,
        seconds): the hits of row row0 + i are the rows j > row0 + i within `radius` bits, by (distance asc, j asc)
        (mi_hamming_self_range).  Capacity as in range_search."""
        lib = load()
        return _range_call(
            self._lock, lambda cap, lims, idx, dist, secs: lib.mi_hamming_self_range(self._h, int(row0), int(nrows), int(radius), cap,
                                                                                     lims, idx, dist, secs),
            int(nrows), max_results, np.int32)

    def get_codes(self, row0=0, nrows=None):
        nrows = self.n - row0 if nrows is None else int(nrows)
        out = np.empty((nrows, self.nbits // 8), dtype=np.uint8)
        with self._lock:
            check(load().mi_hamming_get_codes(self._h, int(row0), nrows, out.ctypes.data_as(C.c_void_p)))
        return out


def component_ids(a, what="ids"):
    """Row ids as mi_components takes them: a contiguous int64 array [m], from integers of any dtype and stride (lists too).
    Raises ValueError on anything that is not a 1-D array of integers; the range [0, n) is the library's to check."""
    a = np.asarray(a)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
        raise ValueError("%s must be a 1-D integer array" % what)
    if a.dtype == np.uint64 and a.size and a.max() > 2 ** 63 - 1:
        raise ValueError("%s must fit int64" % what)
    return np.ascontiguousarray(a, dtype=np.int64)


class Components(_Handle):
    """Connected components of n rows on one MI355X (a `mi_components` handle): a union-find forest of 4 bytes per row, fed with
    the hits of the near-duplicate self-joins.  labels()[v] is the smallest row of v's component, whatever order the edges came
    in -- what Gallery.set_groups takes."""
    _DESTROY = "mi_components_destroy"

    def __init__(self, n, device=0):
        h = C.c_void_p()
        check(load().mi_components_create(int(n), int(device), C.byref(h)))
        super().__init__(h.value)
        self.n, self.device = int(n), int(device)

    def reset(self):
        """Every row a component of its own again."""
        with self._lock:
            check(load().mi_components_reset(self._h))

    def add_pairs(self, i, j):
        """Edges (i[e], j[e]): integer arrays of any integer dtype and stride, or lists.  An id outside [0, n) raises
        RuntimeError and nothing is united."""
        i, j = component_ids(i, "i"), component_ids(j, "j")
        if i.size != j.size:
            raise ValueError("i and j must have the same length")
        with self._lock:
            check(load().mi_components_add_pairs(self._h, C.c_void_p(i.ctypes.data), C.c_void_p(j.ctypes.data), i.size, MI_HOST))

    def add_pairs_device(self, i_ptr, j_ptr, m):
        """m edges in device arrays of int64 (complete when the call is made); ids checked on the device."""
        with self._lock:
            check(load().mi_components_add_pairs(self._h, C.c_void_p(i_ptr), C.c_void_p(j_ptr), int(m), MI_DEVICE))

    def add_csr(self, row0, lims, idx):
        """The CSR output of a self-join: query q is row row0 + q and its hits are idx[lims[q]:lims[q+1]] -- the (lims, ids) of
        Gallery.range_search on stored rows, Gallery.self_range_minkowski or BinaryGallery.self_range (row_offset 0)."""
        lims, idx = component_ids(lims, "lims"), component_ids(idx, "idx")
        if lims.size < 1:
            raise ValueError("lims must hold nq + 1 offsets")
        with self._lock:
            check(load().mi_components_add_csr(self._h, int(row0), C.c_void_p(lims.ctypes.data), C.c_void_p(idx.ctypes.data),
                                               lims.size - 1, MI_HOST))

    def add_csr_device(self, row0, lims_ptr, idx_ptr, nq):
        """lims int64 [nq + 1] and the hits int64 [lims[nq]] in device arrays (complete when the call is made)."""
        with self._lock:
            check(load().mi_components_add_csr(self._h, int(row0), C.c_void_p(lims_ptr), C.c_void_p(idx_ptr), int(nq), MI_DEVICE))

    def add_hamming_self(self, binary, row0, nrows, radius):
        """Unites what binary.self_range(row0, nrows, radius) would report, without any pair being made: `binary` is a
        BinaryGallery or an LSHIndex (its gallery is used) of exactly n codes with row_offset 0 on this device."""
        g = getattr(binary, "gallery", binary)
        with self._lock, g._lock:
            check(load().mi_components_add_hamming_self(self._h, g._h, int(row0), int(nrows), int(radius)))

    def labels(self):
        """-> (labels int32 [n], n_groups): the smallest row of every row's component, and the number of components."""
        out = np.empty(self.n, dtype=np.int32)
        groups = C.c_int64()
        with self._lock:
            check(load().mi_components_labels(self._h, C.c_void_p(out.ctypes.data), MI_HOST, C.byref(groups)))
        return out, groups.value

    def labels_device(self, out_ptr):
        """The labels into a device array of int32 [n] -> n_groups."""
        groups = C.c_int64()
        with self._lock:
            check(load().mi_components_labels(self._h, C.c_void_p(out_ptr), MI_DEVICE, C.byref(groups)))
        return groups.value


LSH_MAX_BITS, LSH_MAX_DIM = 4096, 4096


def _lsh_shape(d, nbits):
    d, nbits = int(d), int(nbits)
    if nbits < 8 or nbits > LSH_MAX_BITS or nbits % 8:
        raise ValueError("n_bits = %d: an LSH code is a multiple of 8 bits in [8, %d]" % (nbits, LSH_MAX_BITS))
    if not 1 <= d <= LSH_MAX_DIM:
        raise ValueError("d = %d: LSH rows have 1 .. %d columns" % (d, LSH_MAX_DIM))
    return d, nbits


def lsh_rotation(d, nbits, seed=5):
    """-> float64 [nbits, d]: the projection directions of an LSH index.  Q of the QR factorisation of an m x m standard normal
    matrix drawn by RandomState(seed), m = max(d, nbits), cut to its first nbits rows and d columns: orthonormal rows when
    nbits <= d.  This is the construction of faiss's RandomRotationMatrix, which IndexLSH(d, nbits) initialises with the same
    seed 5 -- but not faiss's random stream (its own generator, float32), so the directions differ from faiss's the way two
    seeds differ.  Deterministic: two calls return equal bits."""
    d, nbits = _lsh_shape(d, nbits)
    m = max(d, nbits)
    q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((m, m)))
    return np.ascontiguousarray(q[:nbits, :d], dtype=np.float64)


def _lsh_operands(d, R, thresholds):
    """R float64 [nbits, d] C-contiguous and the thresholds float64 [nbits] (or None) of rows of d columns."""
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.ndim != 2 or R.shape[1] != int(d):
        raise ValueError("R must be [nbits, d = %d] (got %s)" % (d, R.shape))
    _lsh_shape(d, R.shape[0])
    t = None
    if thresholds is not None:
        t = np.ascontiguousarray(thresholds, dtype=np.float64)
        if t.shape != (R.shape[0],):
            raise ValueError("thresholds must be [nbits = %d] (got %s)" % (R.shape[0], t.shape))
    return R, t


def lsh_encode(x, R, thresholds=None, device=0):
    """Rows x [n, d] float32/float64 (any strides) -> LSH codes uint8 [n, nbits / 8]: bit j = (x . R[j] >= thresholds[j]), the
    sum in float64, thresholds None = 0 (mi_lsh_encode; faiss IndexLSH's sa_encode without trained thresholds).  Host in, host
    out; the rows pass through the device in blocks."""
    a, code, rs, cs = _strided(x)
    R, t = _lsh_operands(a.shape[1], R, thresholds)
    out = np.empty((a.shape[0], R.shape[0] // 8), dtype=np.uint8)
    check(load().mi_lsh_encode(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs, C.c_void_p(R.ctypes.data),
                               None if t is None else C.c_void_p(t.ctypes.data), R.shape[0], device,
                               out.ctypes.data_as(C.c_void_p)))
    return out


def lsh_encode_device(x_ptr, n, d, r_ptr, nbits, out_ptr, thr_ptr=None, dtype=MI_F32, row_stride=None, col_stride=1,
                      out_row_stride=None, stream=None):
    """Device rows [n][d] -> LSH codes [n][nbits / 8] uint8 on the device, enqueued on `stream` (mi_lsh_encode_device)."""
    check(load().mi_lsh_encode_device(C.c_void_p(x_ptr), int(n), int(d), dtype, int(d if row_stride is None else row_stride),
                                      int(col_stride), C.c_void_p(r_ptr), C.c_void_p(thr_ptr), int(nbits), C.c_void_p(out_ptr),
                                      int(nbits // 8 if out_row_stride is None else out_row_stride), C.c_void_p(stream)))


class LSHIndex(_Closing):
    """LSH index on one MI355X, faiss IndexLSH(d, nbits) without trained thresholds: a BinaryGallery of the codes
    bit j = (x . R[j] >= thresholds[j]) plus R float64 [nbits, d] and the thresholds on the device.  Rows are encoded straight
    into the gallery's code storage; a search encodes its queries on the device and runs the exact Hamming top-k there, by
    (distance asc, id asc)."""

    def __init__(self, gallery, R, thresholds=None):
        import torch
        R, t = _lsh_operands(np.shape(R)[1], R, thresholds)
        if R.shape[0] != gallery.nbits:
            raise ValueError("R has %d rows, the gallery holds codes of %d bits" % (R.shape[0], gallery.nbits))
        self.gallery, self.R, self.thresholds = gallery, R, t
        self.nbits, self.d = R.shape
        self.device = gallery.device
        self._tdev = "cuda:%d" % gallery.device
        self._R = torch.from_numpy(R).to(self._tdev)
        self._thr = None if t is None else torch.from_numpy(t).to(self._tdev)

    @classmethod
    def empty(cls, d, nbits, capacity, R=None, thresholds=None, seed=5, device=0, row_offset=0):
        """Appendable index of `capacity` rows.  R None: lsh_rotation(d, nbits, seed)."""
        if R is None:
            if nbits is None:
                raise ValueError("give nbits or R")
            R = lsh_rotation(d, nbits, seed)
        R, t = _lsh_operands(d, R, thresholds)
        if nbits is not None and int(nbits) != R.shape[0]:
            raise ValueError("nbits = %d, R has %d rows" % (nbits, R.shape[0]))
        if int(capacity) < 1:
            raise ValueError("an empty index needs a capacity")
        return cls(BinaryGallery.empty(int(capacity), R.shape[0], device=device, row_offset=row_offset), R, t)

    @classmethod
    def from_host(cls, x, nbits=None, R=None, thresholds=None, seed=5, device=0, capacity=0):
        """Index of the rows x [N, d] float32/float64; capacity 0 = N, larger leaves room for add()."""
        a, _, _, _ = _strided(x)
        if capacity and capacity < a.shape[0]:
            raise ValueError("capacity %d below the %d rows given" % (capacity, a.shape[0]))
        idx = cls.empty(a.shape[1], nbits, capacity or a.shape[0], R=R, thresholds=thresholds, seed=seed, device=device)
        idx.add(a)
        return idx

    @property
    def n(self):
        return self.gallery.n

    @property
    def capacity(self):
        return self.gallery.capacity

    @property
    def hbm_bytes(self):
        return self.gallery.hbm_bytes + self.R.nbytes + (0 if self.thresholds is None else self.thresholds.nbytes)

    def _rows(self, x):
        a, code, _, _ = _strided(x)
        if a.shape[1] != self.d:
            raise ValueError("rows of %d columns, the index takes %d" % (a.shape[1], self.d))
        return a, code

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._tdev).cuda_stream

    def _thr_ptr(self):
        return None if self._thr is None else self._thr.data_ptr()

    def _blocks(self, a):
        """Host rows -> (first row, packed device rows) in blocks of at most 64 MiB."""
        import torch
        step = max(128, (64 << 20) // (self.d * a.dtype.itemsize))
        for r in range(0, a.shape[0], step):
            yield r, torch.from_numpy(np.ascontiguousarray(a[r:r + step])).to(self._tdev)

    def add(self, x):
        """Encodes host rows [rows, d] float32/float64 (any strides) on the device and appends their codes; synchronous."""
        import torch
        a, code = self._rows(x)
        if self.gallery.n + a.shape[0] > self.gallery.capacity:
            raise ValueError("%d rows more than the capacity %d holds (%d are in)" % (a.shape[0], self.gallery.capacity, self.gallery.n))
        for _, blk in self._blocks(a):
            self.gallery.append_lsh_device(blk.data_ptr(), blk.shape[0], self.d, self._R.data_ptr(), self._thr_ptr(), dtype=code,
                                           stream=self._stream())
        torch.cuda.current_stream(self._tdev).synchronize()

    def add_device(self, x_ptr, rows, dtype=MI_F32, row_stride=None, col_stride=1, stream=None):
        """Device rows, enqueued on `stream` without synchronising (mi_hamming_append_lsh_device)."""
        self.gallery.append_lsh_device(x_ptr, rows, self.d, self._R.data_ptr(), self._thr_ptr(), dtype=dtype, row_stride=row_stride,
                                       col_stride=col_stride, stream=stream)

    def encode(self, q):
        """-> codes uint8 [rows, nbits / 8] of host rows, computed on the device.  The index is unchanged."""
        import torch
        a, code = self._rows(q)
        out = np.empty((a.shape[0], self.nbits // 8), dtype=np.uint8)
        for r, blk in self._blocks(a):
            codes = torch.empty((blk.shape[0], self.nbits // 8), dtype=torch.uint8, device=self._tdev)
            lsh_encode_device(blk.data_ptr(), blk.shape[0], self.d, self._R.data_ptr(), self.nbits, codes.data_ptr(),
                              thr_ptr=self._thr_ptr(), dtype=code, stream=self._stream())
            out[r:r + blk.shape[0]] = codes.cpu().numpy()
        return out

    def _encode_on_device(self, a, code, stream):
        """Host rows [rows, d] of dtype `code` (or a tensor of them already on the device) -> (the device rows, their codes uint8
        [rows, nbits / 8] on the device), the encoding enqueued on `stream`."""
        import torch
        xq = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(self._tdev)
        qcodes = torch.empty((xq.shape[0], self.nbits // 8), dtype=torch.uint8, device=self._tdev)
        lsh_encode_device(xq.data_ptr(), xq.shape[0], self.d, self._R.data_ptr(), self.nbits, qcodes.data_ptr(),
                          thr_ptr=self._thr_ptr(), dtype=code, stream=stream)
        return xq, qcodes

    def search(self, q, k, allow=None, refine=None, k_factor=1):
        """refine=<Gallery of the raw rows>: the Hamming search takes refine_kc(k, k_factor, n) ids, the gallery re-ranks them on
        the device (Gallery.refine) and the distances returned are its exact float32 values.  Otherwise:
        -> (ids int64 [Q,k], dist int32 [Q,k], seconds), ordered by (Hamming distance asc, id asc).  The queries are encoded on
        the device and searched there (mi_lsh_encode_device, mi_hamming_search_device): only the queries, the allow bitmap and
        the answer cross the host link.  allow: anything allow_bitmap takes.  Fewer than k admitted rows: trailing ids -1,
        distances INT32_MAX.  seconds: wall time of upload, encoding, search and download, device-synchronised."""
        import torch
        a, code = self._rows(q)
        nq, k = a.shape[0], int(k)
        if not 1 <= k <= 2048:
            raise ValueError("k must be in [1, 2048]")
        bits = _allow_words(allow, self.gallery.n, self.gallery.row_offset)
        if refine is not None:
            return _search_refined(refine, np.ascontiguousarray(a, dtype=np.float32), k, refine_kc(k, k_factor, self.gallery.n),
                                   (bits, None, MI_HOST), self.device, None, self.gallery.search_device,
                                   stage=lambda xq, stream: (self._encode_on_device(xq, MI_F32, stream)[1], {}))
        if nq == 0:
            return np.empty((0, k), np.int64), np.empty((0, k), np.int32), 0.0
        t0 = time.perf_counter()
        stream = self._stream()
        xq, qcodes = self._encode_on_device(a, code, stream)
        bits_dev = _upload_allow(bits, self._tdev)
        idx = torch.empty((nq, k), dtype=torch.int64, device=self._tdev)
        dist = torch.empty((nq, k), dtype=torch.int32, device=self._tdev)
        self.gallery.search_device(qcodes.data_ptr(), nq, k, idx.data_ptr(), dist_ptr=dist.data_ptr(),
                                   allow_ptr=None if bits_dev is None else bits_dev.data_ptr(), stream=stream)
        ids, dd = idx.cpu().numpy(), dist.cpu().numpy()              # (synchronises with the stream the work is on)
        return ids, dd, time.perf_counter() - t0

    def range_search(self, q, radius, allow=None, max_results=None):
        """-> (lims int64 [Q+1], ids int64, dist int32, seconds): every admitted row whose code is within `radius` bits
        (inclusive) of the query's, per query by (distance asc, id asc).  The queries are encoded on the device and searched there
        (mi_lsh_encode_device, mi_hamming_range_search_device).  The first capacity is `max_results` (default Q * 1024); if the
        hits do not fit, the search runs once more with exactly lims[-1]."""
        import torch
        a, code = self._rows(q)
        nq = a.shape[0]
        if int(radius) < 0:
            raise ValueError("radius must be >= 0")
        if nq == 0:
            return np.zeros(1, np.int64), np.empty(0, np.int64), np.empty(0, np.int32), 0.0
        bits = _allow_words(allow, self.gallery.n, self.gallery.row_offset)
        t0 = time.perf_counter()
        stream = self._stream()
        xq, qcodes = self._encode_on_device(a, code, stream)
        bits_dev = _upload_allow(bits, self._tdev)
        lims = torch.empty(nq + 1, dtype=torch.int64, device=self._tdev)
        cap = _range_capacity(nq, max_results)
        for attempt in range(2):
            idx = torch.empty(max(cap, 1), dtype=torch.int64, device=self._tdev)
            dist = torch.empty(max(cap, 1), dtype=torch.int32, device=self._tdev)
            with self.gallery._lock:
                self.gallery.range_search_device(qcodes.data_ptr(), nq, radius, cap, lims.data_ptr(), idx.data_ptr(),
                                                 dist_ptr=dist.data_ptr(),
                                                 allow_ptr=None if bits_dev is None else bits_dev.data_ptr(), stream=stream)
            lims_h = lims.cpu().numpy()                                  # (synchronises with the stream the work is on)
            total = int(lims_h[-1])
            if total <= cap:
                break
            cap = total
        return lims_h, idx[:total].cpu().numpy(), dist[:total].cpu().numpy(), time.perf_counter() - t0

    def get_codes(self, row0=0, nrows=None):
        return self.gallery.get_codes(row0, nrows)

    def close(self):
        if self.gallery is not None:
            self.gallery.close()
            self.gallery = self._R = self._thr = None


PQ_MAX_BOOKS, PQ_MAX_WORDS, PQ_MAX_DIM = 64, 256, 4096
PQW_MAX_WORDS = 8192              # the wide index (WidePQIndex, mi_pqw): uint16 codes
PQW_SLAB_ROWS = 16384             # the most rows one workgroup of its scan walks (csrc/pq_wide.hip: 64 * PW_WAVES * PW_RPL)


def _pq_check_words(ks, max_words):
    if not 2 <= ks <= max_words:
        if max_words == PQ_MAX_WORDS:
            raise ValueError("Ks = %d codewords per book, a PQ index takes 2 .. %d (one byte per book)" % (ks, max_words))
        raise ValueError("Ks = %d codewords per book, a wide PQ index takes 2 .. %d" % (ks, max_words))


def pq_codebooks(codebooks, max_words=PQ_MAX_WORDS):
    """float32 [M, Ks, L] C-contiguous codebooks (nanopq's pq.codewords, faiss's ProductQuantizer.centroids), checked against
    what a PQ index takes: 1 <= M <= 64, 2 <= Ks <= 256 (max_words; PQW_MAX_WORDS for the wide index), M * L <= 4096, finite.
    Raises ValueError."""
    cb = np.ascontiguousarray(codebooks, dtype=np.float32)
    if cb.ndim != 3:
        raise ValueError("codebooks must be [M, Ks, L] (got shape %s)" % (cb.shape,))
    m, ks, L = cb.shape
    if not 1 <= m <= PQ_MAX_BOOKS:
        raise ValueError("M = %d books, a PQ index takes 1 .. %d" % (m, PQ_MAX_BOOKS))
    _pq_check_words(ks, max_words)
    if L < 1 or m * L > PQ_MAX_DIM:
        raise ValueError("d = M * L = %d, a PQ index takes 1 .. %d" % (m * L, PQ_MAX_DIM))
    if not np.isfinite(cb).all():
        raise ValueError("codebooks must be finite")
    return cb


def pq_code_rows(codes, m, ks, dtype=np.uint8):
    """uint8 [rows, m] code rows (dtype: uint16 for the wide index) from any integer array with values in [0, ks) (row stride kept
    when the array has that type and contiguous rows) -> (rows, row stride in elements).  Raises ValueError on another dtype,
    shape or a value outside [0, ks)."""
    a = np.asarray(codes)
    if a.ndim != 2 or a.shape[1] != m:
        raise ValueError("codes must be [rows, M = %d] (got shape %s)" % (m, a.shape))
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("codes must be an integer array of codeword indices (got %s)" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= ks):
        raise ValueError("codes must lie in [0, Ks = %d)" % ks)
    size = np.dtype(dtype).itemsize
    if a.dtype != dtype:
        a = a.astype(dtype)
    if a.shape[1] > 1 and a.strides[1] != size or a.strides[0] < a.shape[1] * size or a.strides[0] % size:
        a = np.ascontiguousarray(a)
    return a, max(int(a.strides[0]) // size, a.shape[1])


def _pq_train_shape(n, d, M, Ks, iters, max_words=PQ_MAX_WORDS):
    """The limits of mi_pq_train (max_words = PQW_MAX_WORDS: of mi_pqw_train), answered with ValueError before the library is
    loaded.  -> L"""
    n, d, M, Ks, iters = int(n), int(d), int(M), int(Ks), int(iters)
    if not 1 <= M <= PQ_MAX_BOOKS:
        raise ValueError("M = %d books, a PQ index takes 1 .. %d" % (M, PQ_MAX_BOOKS))
    _pq_check_words(Ks, max_words)
    if not 1 <= d <= PQ_MAX_DIM:
        raise ValueError("d = %d, a PQ index takes 1 .. %d" % (d, PQ_MAX_DIM))
    if d % M:
        raise ValueError("d = %d is no multiple of M = %d" % (d, M))
    if n < Ks:
        raise ValueError("n = %d training rows, Ks = %d codewords need at least as many" % (n, Ks))
    if iters < 1:
        raise ValueError("iters = %d, training takes at least one iteration" % iters)
    return d // M


def _pq_train_init(init, M, Ks, L, max_words=PQ_MAX_WORDS):
    cb = pq_codebooks(init, max_words)
    if cb.shape != (M, Ks, L):
        raise ValueError("init of shape %s, the training takes [M, Ks, L] = %s" % (cb.shape, (M, Ks, L)))
    return cb


def _pq_train_call(ptr, n, d, code, rs, cs, memspace, M, Ks, iters, cb0, device, fn="mi_pq_train"):
    L = d // M
    out = np.empty((M, Ks, L), dtype=np.float32)
    moved = np.zeros(iters, dtype=np.int64)
    check(getattr(load(), fn)(C.c_void_p(ptr), int(n), int(d), code, int(rs), int(cs), memspace, M, Ks, iters,
                              None if cb0 is None else C.c_void_p(cb0.ctypes.data), device, out.ctypes.data_as(C.c_void_p),
                              moved.ctypes.data_as(C.c_void_p), None))
    return out, moved


def pq_train(x, M, Ks, iters=20, init=None, init_rows=None, seed=None, device=0, _max_words=PQ_MAX_WORDS, _fn="mi_pq_train"):
    """Learns PQ codebooks on the device (mi_pq_train): Lloyd's k-means iteration per book, as a deterministic function of its
    inputs.  x [n, d] float32/float64 (any strides), n >= Ks -> (codebooks float32 [M, Ks, L], moved int64 [iters]).
    The initial codebooks are ONE of
      init       a codebook array [M, Ks, L] (a result passed back in resumes the run bit for bit);
      init_rows  an integer array [M, Ks] of row indices: codeword c of book j starts as book j's slice of row init_rows[j, c],
                 gathered on the host;
      seed       init_rows drawn as RandomState(seed).choice(n, Ks, replace=False), once per book in book order from one
                 RandomState;
    or, with none of them, the library's default: the rows floor(c * n / Ks).  More than one given is a ValueError.
    moved[t] counts the (row, book) pairs whose codeword changed in iteration t (moved[0] = n * M); training stops at the first
    zero and the remaining entries stay zero.  Arithmetic: float64 argmin assignment with ties to the lower codeword, member sums
    in float64 in ascending row order, one divide, centroids rounded to float32 after every iteration; a codeword without members
    keeps its value -- scipy.cluster.vq.kmeans2(minit="matrix"), the routine nanopq.PQ.fit runs per book.  It does NOT reproduce
    nanopq's or faiss's random draw of initial points, nor their float32 arithmetic.  Bad arguments and non-finite rows raise
    ValueError before the device is touched."""
    a, code, rs, cs, cb0 = _pq_train_operands(x, M, Ks, iters, init, init_rows, seed, _max_words)
    return _pq_train_call(_base_pointer(a), a.shape[0], a.shape[1], code, rs, cs, MI_HOST, int(M), int(Ks), int(iters), cb0, device, _fn)


def _pq_train_operands(x, M, Ks, iters, init, init_rows, seed, max_words):
    """What pq_train checks and prepares before the library is loaded -> (rows, dtype code, row stride, col stride, C_0 or None)."""
    a, code, rs, cs = _strided(x)
    n, d = a.shape
    M, Ks, iters = int(M), int(Ks), int(iters)
    L = _pq_train_shape(n, d, M, Ks, iters, max_words)
    if (init is not None) + (init_rows is not None) + (seed is not None) > 1:
        raise ValueError("give at most one of init, init_rows and seed")
    if not np.isfinite(a).all():
        raise ValueError("training rows must be finite")
    cb0 = None
    if init is not None:
        cb0 = _pq_train_init(init, M, Ks, L, max_words)
    elif seed is not None:
        rng = np.random.RandomState(seed)
        init_rows = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
    if init_rows is not None:
        rows = np.asarray(init_rows)
        if rows.shape != (M, Ks) or rows.dtype == np.bool_ or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("init_rows must be an integer array [M, Ks] = %s (got %s %s)" % ((M, Ks), rows.dtype, rows.shape))
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= n):
            raise ValueError("init_rows must lie in [0, n = %d)" % n)
        cb0 = np.ascontiguousarray(np.stack([a[rows[j], j * L:(j + 1) * L] for j in range(M)]), dtype=np.float32)
    return a, code, rs, cs, cb0


def pq_train_device(x_ptr, n, d, M, Ks, iters, init=None, dtype=MI_F32, row_stride=None, col_stride=1, device=0,
                    _max_words=PQ_MAX_WORDS, _fn="mi_pq_train"):
    """pq_train on device-resident rows (used where they lie; their producer must have completed): element (r, i) at
    x_ptr + (r * row_stride + i * col_stride) elements of `dtype`, row_stride None = d.  init: codebooks [M, Ks, L] or None (the
    rows floor(c * n / Ks)).  Non-finite rows leave the codebooks of the books they touch unspecified."""
    M, Ks, iters = int(M), int(Ks), int(iters)
    L = _pq_train_shape(n, d, M, Ks, iters, _max_words)
    cb0 = None if init is None else _pq_train_init(init, M, Ks, L, _max_words)
    return _pq_train_call(int(x_ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride, MI_DEVICE, M, Ks, iters, cb0,
                          device, _fn)


def pqw_train(x, M, Ks, iters=20, init=None, init_rows=None, seed=None, device=0):
    """pq_train with 2 <= Ks <= PQW_MAX_WORDS = 8192 (mi_pqw_train): the same arguments, the same iteration, the same bits -- for
    Ks <= 256 the result equals pq_train's.  The codebooks of a WidePQIndex."""
    return pq_train(x, M, Ks, iters, init, init_rows, seed, device, _max_words=PQW_MAX_WORDS, _fn="mi_pqw_train")


def pqw_train_device(x_ptr, n, d, M, Ks, iters, init=None, dtype=MI_F32, row_stride=None, col_stride=1, device=0):
    """pq_train_device with 2 <= Ks <= PQW_MAX_WORDS (mi_pqw_train)."""
    return pq_train_device(x_ptr, n, d, M, Ks, iters, init, dtype, row_stride, col_stride, device, _max_words=PQW_MAX_WORDS,
                           _fn="mi_pqw_train")


def pq_train_timing():
    """-> (assign_ms float32 [iterations that ran], update_ms float32 [updates that ran]): device times of this thread's last
    pq_train / pq_train_device call."""
    na, nu = C.c_int32(), C.c_int32()
    check(load().mi_pq_train_timing(0, None, None, C.byref(na), C.byref(nu)))
    cap = max(na.value, nu.value, 1)
    a, u = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    check(load().mi_pq_train_timing(cap, a.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), None, None))
    return a[:na.value], u[:nu.value]


KMEANS_MAX_CLUSTERS = PQW_MAX_WORDS  # centroids of kmeans_train / kmeans_assign (mi_kmeans_*)


def _kmeans_call(ptr, n, d, code, rs, cs, memspace, k, iters, cb0, device, return_flagged):
    out = np.empty((k, d), dtype=np.float32)
    moved, flagged = np.zeros(iters, dtype=np.int64), np.zeros(iters, dtype=np.int64)
    check(load().mi_kmeans_train(C.c_void_p(ptr), int(n), int(d), code, int(rs), int(cs), memspace, k, iters,
                                 None if cb0 is None else C.c_void_p(cb0.ctypes.data), device, out.ctypes.data_as(C.c_void_p),
                                 moved.ctypes.data_as(C.c_void_p), flagged.ctypes.data_as(C.c_void_p), None))
    return (out, moved, flagged) if return_flagged else (out, moved)


def _kmeans_book(a, what):
    """A centroid array [k, d] or row-index array [k] in pq_train's one-book shape, [1, k, d] or [1, k]."""
    if a is None:
        return None
    a = np.asarray(a)
    return a[None] if a.ndim == what else a


def kmeans_train(x, k, iters=20, init=None, init_rows=None, seed=None, device=0, return_flagged=False):
    """k-means over whole rows on the device (mi_kmeans_train): Lloyd's iteration with k centroids of d floats, 2 <= k <= 8192 ->
    (centroids float32 [k, d], moved int64 [iters]), bit for bit pqw_train(x, 1, k, ...)'s codebook and move counts -- the same
    contract, init rules (init [k, d], init_rows [k], seed, or the rows floor(c * n / k)) and ValueErrors with M = 1.  The
    assignment runs at f64 matrix rate: an MFMA kernel decides every row whose two best centroids lie further apart than a
    rounding bound, the direct-form arithmetic the rest.  return_flagged=True appends flagged int64 [iters], the rows per
    iteration the second kind decided.  pq_train_timing reports this call too."""
    a, code, rs, cs, cb0 = _pq_train_operands(x, 1, k, iters, _kmeans_book(init, 2), _kmeans_book(init_rows, 1), seed, KMEANS_MAX_CLUSTERS)
    return _kmeans_call(_base_pointer(a), a.shape[0], a.shape[1], code, rs, cs, MI_HOST, int(k), int(iters), cb0, device,
                        return_flagged)


def kmeans_train_device(x_ptr, n, d, k, iters, init=None, dtype=MI_F32, row_stride=None, col_stride=1, device=0,
                        return_flagged=False):
    """kmeans_train on device-resident rows (used where they lie; their producer must have completed), addressed as in
    pq_train_device.  init: centroids [k, d] or None (the rows floor(c * n / k))."""
    k, iters = int(k), int(iters)
    _pq_train_shape(n, d, 1, k, iters, KMEANS_MAX_CLUSTERS)
    cb0 = None if init is None else _pq_train_init(_kmeans_book(init, 2), 1, k, int(d), KMEANS_MAX_CLUSTERS)
    return _kmeans_call(int(x_ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride, MI_DEVICE, k, iters, cb0,
                        device, return_flagged)


def kmeans_centroids(centroids, d=None):
    """float32 [k, d] C-contiguous centroids, checked against what kmeans_assign takes: 2 <= k <= 8192, d <= 4096, finite.  Raises
    ValueError."""
    g = np.asarray(centroids)
    if g.ndim == 3 and g.shape[0] == 1:              # what pq_train(x, 1, k) returns
        g = g[0]
    g = pq_codebooks(g[None] if g.ndim == 2 else g, KMEANS_MAX_CLUSTERS)[0]
    if d is not None and g.shape[1] != int(d):
        raise ValueError("centroids of %d columns, the rows have d = %d" % (g.shape[1], d))
    return g


def kmeans_assign(x, centroids, device=0, return_flagged=False):
    """-> int32 [n]: the id of every row's nearest centroid (mi_kmeans_assign), the float64 direct-form argmin with ties to the
    lower id -- what WidePQIndex.encode returns on a one-book index holding `centroids` [k, d].  Host in, host out; the rows pass
    through the device in bounded blocks.  return_flagged=True -> (ids, the number of rows the direct-form kernel decided)."""
    a, code, rs, cs = _strided(x)
    g = kmeans_centroids(centroids, a.shape[1])
    if not np.isfinite(a).all():
        raise ValueError("rows must be finite")
    out = np.empty(a.shape[0], dtype=np.int32)
    flagged = C.c_int64()
    check(load().mi_kmeans_assign(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs, C.c_void_p(g.ctypes.data),
                                  g.shape[0], device, out.ctypes.data_as(C.c_void_p), C.byref(flagged)))
    return (out, flagged.value) if return_flagged else out


def kmeans_assign_workspace_bytes(k, n):
    """Bytes of device workspace kmeans_assign_device uses for n rows and k centroids (at most 64 MiB and a little)."""
    _pq_check_words(int(k), KMEANS_MAX_CLUSTERS)
    b = C.c_int64()
    check(load().mi_kmeans_assign_workspace_bytes(int(k), int(n), C.byref(b)))
    return b.value


def kmeans_assign_device(x_ptr, n, d, centroids_ptr, k, out_ptr, workspace_ptr, workspace_bytes, flagged_ptr=None, dtype=MI_F32,
                         row_stride=None, col_stride=1, stream=None):
    """Device rows [n][d] and float32 centroids [k][d] -> int32 ids [n] on the device, enqueued on `stream` with no
    synchronisation and nothing read back (mi_kmeans_assign_device).  flagged_ptr: an optional device uint64 that receives the
    number of rows the direct-form kernel decided.  The workspace (kmeans_assign_workspace_bytes) is the caller's and stays
    untouched by others until the work on `stream` is done."""
    check(load().mi_kmeans_assign_device(C.c_void_p(x_ptr), int(n), int(d), dtype, int(d if row_stride is None else row_stride),
                                         int(col_stride), C.c_void_p(centroids_ptr), int(k), C.c_void_p(out_ptr),
                                         C.c_void_p(flagged_ptr), C.c_void_p(workspace_ptr), int(workspace_bytes),
                                         C.c_void_p(stream)))


class KMeans:
    """The members the reference uses of sklearn.cluster.KMeans (src/utils/nnsearch.py:967-989) on kmeans_train / kmeans_assign:
    fit(x) draws the initial rows as RandomState(seed).choice(n, n_clusters, replace=False) and leaves cluster_centers_ float32
    [n_clusters, d], labels_ int32 [n] (the assignment under the final centroids) and n_iter_; predict(x) -> int32 ids.
    Deterministic; it is Lloyd's iteration in float64 as kmeans_train states it, not sklearn's k-means++ or its tolerance."""

    def __init__(self, n_clusters, iters=20, seed=0, device=0):
        self.n_clusters, self.iters, self.seed, self.device = int(n_clusters), int(iters), seed, device
        _pq_check_words(self.n_clusters, KMEANS_MAX_CLUSTERS)
        if self.iters < 1:
            raise ValueError("iters = %d, training takes at least one iteration" % self.iters)
        self.cluster_centers_ = self.labels_ = self.n_iter_ = None

    def fit(self, x):
        c, moved = kmeans_train(x, self.n_clusters, iters=self.iters, seed=self.seed, device=self.device)
        stops = np.flatnonzero(moved[1:] == 0)
        self.n_iter_ = int(stops[0]) + 2 if stops.size else self.iters      # iterations that assigned (the stopping one included)
        self.cluster_centers_ = c
        self.labels_ = kmeans_assign(x, c, device=self.device)
        return self

    def predict(self, x):
        if self.cluster_centers_ is None:
            raise ValueError("predict before fit: the KMeans has no centroids yet")
        return kmeans_assign(x, self.cluster_centers_, device=self.device)


def _remove_rows(index, name, rows):
    """Gallery.remove for a PQIndex / IVFPQIndex: the bitmap of `rows`, the call `name` of the library, `kept`, index.n."""
    bits = _allow_words(rows, index.n, index.row_offset)      # (an empty index: one zero word)
    gone = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), bitorder="little")[:index.n].astype(np.bool_)
    kept = np.flatnonzero(~gone).astype(np.int64) + int(index.row_offset)
    removed = C.c_int64()
    with index._lock:
        check(getattr(load(), name)(index._h, C.c_void_p(bits.ctypes.data), MI_HOST, C.byref(removed)))
        if index.n - removed.value != kept.size:
            raise RuntimeError("%s removed %d rows, the bitmap names %d" % (name, removed.value, index.n - kept.size))
        index.n = int(kept.size)
    return kept


class _PQBase(_Handle):
    """What PQIndex (`mi_pq`, byte codes) and WidePQIndex (`mi_pqw`, uint16 codes) share: every entry point but row removal, the
    library's names behind `_PREFIX`, the code type and the limit on Ks class attributes."""
    _PREFIX = _CODE = _MAX_WORDS = _TRAIN = None

    @classmethod
    def _fn(cls, name):
        return getattr(load(), "%s_%s" % (cls._PREFIX, name))

    def __init__(self, handle):
        super().__init__(handle)
        n, cap, off, hb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        d, m, ks, dev = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self._fn("info")(self._h, n, d, m, ks, dev, off, cap, hb))
        self.n, self.d, self.m, self.ks, self.device = n.value, d.value, m.value, ks.value, dev.value
        self.row_offset, self.capacity = off.value, cap.value

    @classmethod
    def _create(cls, cb, ptr, n, stride, memspace, device, row_offset, capacity):
        m, ks, L = cb.shape
        h = C.c_void_p()
        check(cls._fn("create")(C.c_void_p(cb.ctypes.data), m * L, m, ks, C.c_void_p(ptr), int(n), int(stride), memspace, device,
                                  int(row_offset), int(capacity), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_codes(cls, codebooks, codes, device=0, row_offset=0, capacity=0):
        """codebooks [M, Ks, L] float32, codes integer [N, M] with values in [0, Ks); capacity 0 = N, larger leaves room for
        append_codes() / add()."""
        cb = pq_codebooks(codebooks, cls._MAX_WORDS)
        a, stride = pq_code_rows(codes, cb.shape[0], cb.shape[1], cls._CODE)
        if capacity and capacity < a.shape[0]:
            raise ValueError("capacity %d below the %d rows given" % (capacity, a.shape[0]))
        return cls._create(cb, a.ctypes.data, a.shape[0], stride, MI_HOST, device, row_offset, capacity)

    @classmethod
    def from_device_ptr(cls, codebooks, ptr, n, device=0, row_offset=0, capacity=0, row_stride_bytes=None, row_stride=None):
        """Device codes [n][M] of the index's code type -> index, synchronous; the producer of `ptr` must have completed.  The
        distance between two rows: row_stride_bytes (PQIndex: bytes) or row_stride (WidePQIndex: uint16 elements), None = M."""
        cb = pq_codebooks(codebooks, cls._MAX_WORDS)
        stride = row_stride_bytes if cls._CODE is np.uint8 else row_stride
        return cls._create(cb, ptr, n, cb.shape[0] if stride is None else stride, MI_DEVICE, device, row_offset, capacity)

    @classmethod
    def empty(cls, codebooks, capacity, device=0, row_offset=0):
        """Appendable index: `capacity` rows allocated, filled by append_codes() / add()."""
        cb = pq_codebooks(codebooks, cls._MAX_WORDS)
        if int(capacity) < 1:
            raise ValueError("an empty index needs a capacity")
        return cls._create(cb, None, 0, cb.shape[0], MI_HOST, device, row_offset, capacity)

    @classmethod
    def fit(cls, x, M, Ks, iters=20, seed=42, capacity=0, device=0, row_offset=0):
        """Learns the codebooks on x [n, d] (pq_train with `seed`; seed=None: the library's default initial rows), creates the
        index and adds x.  The move counts of the training are in `.train_moved`."""
        cb, moved = cls._TRAIN(x, M, Ks, iters=iters, seed=seed, device=device)
        n = np.shape(x)[0]
        if capacity and capacity < n:
            raise ValueError("capacity %d below the %d rows given" % (capacity, n))
        idx = cls.empty(cb, capacity or n, device=device, row_offset=row_offset)
        idx.train_moved = moved
        idx.add(x)
        return idx

    @property
    def codebooks(self):
        out = np.empty((self.m, self.ks, self.d // self.m), dtype=np.float32)
        check(self._fn("get_codebooks")(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def _rows(self, x):
        a, code, rs, cs = _strided(x)
        if a.shape[1] != self.d:
            raise ValueError("rows of %d columns, the index takes %d" % (a.shape[1], self.d))
        return a, code, rs, cs

    def append_codes(self, codes):
        a, stride = pq_code_rows(codes, self.m, self.ks, self._CODE)
        with self._lock:
            check(self._fn("append_codes")(self._h, C.c_void_p(a.ctypes.data), a.shape[0], stride, MI_HOST))
            self.n += a.shape[0]

    def add(self, x):
        """Encodes rows [rows, d] float32/float64 (any strides) on the device and appends their codes."""
        a, code, rs, cs = self._rows(x)
        with self._lock:
            check(self._fn("add")(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST))
            self.n += a.shape[0]

    def add_device(self, x_ptr, rows, dtype=MI_F32, row_stride=None, col_stride=1):
        with self._lock:
            check(self._fn("add")(self._h, C.c_void_p(x_ptr), int(rows), dtype, self.d if row_stride is None else int(row_stride),
                                   int(col_stride), MI_DEVICE))
            self.n += int(rows)

    def encode(self, x):
        """-> codes [rows, M] of the index's code type: per book the codeword nearest in float64, ties to the lower index.  The index is unchanged."""
        a, code, rs, cs = self._rows(x)
        out = np.empty((a.shape[0], self.m), dtype=self._CODE)
        with self._lock:
            check(self._fn("encode")(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST,
                                      out.ctypes.data_as(C.c_void_p)))
        return out

    def dtable(self, q):
        """-> float32 [Q, M, Ks]: squared distances of the queries' sub-vectors to every codeword (nanopq's dtable)."""
        a, code, rs, cs = self._rows(q)
        out = np.empty((a.shape[0], self.m, self.ks), dtype=np.float32)
        with self._lock:
            check(self._fn("dtable")(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, out.ctypes.data_as(C.c_void_p)))
        return out

    def search(self, q, k, allow=None, allow_ptr=None, refine=None, k_factor=1):
        """-> (ids int64 [Q,k], dist float32 [Q,k], seconds), ordered by (distance asc, id asc).  allow: anything allow_bitmap
        takes (bool mask, global ids, AllowBits words); allow_ptr: a device bitmap of ceil(n / 64) uint64 words.  Fewer than k
        admitted rows: trailing ids -1, distances +inf.
        refine=<Gallery of the raw rows>: the ADC search takes refine_kc(k, k_factor, n) ids on the device, the gallery re-ranks
        them there (Gallery.refine; queries rounded to float32) and the distances returned are its exact float32 values."""
        a, code, rs, cs = self._rows(q)
        nq, k = a.shape[0], int(k)
        resolved = bits, bits_p, memspace = _resolve_allow(allow, allow_ptr, self.n, self.row_offset)
        if refine is not None:
            return _search_refined(refine, a, k, refine_kc(k, k_factor, self.n), resolved, self.device, self._lock, self.search_device)
        return self._topk(nq, k, (np.float32,), lambda idx, dist, secs: self._fn("search")(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, bits_p, memspace, idx, dist, secs))

    def search_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, allow_ptr=None, stream=None):
        """q_ptr: packed float32 [nq][d] on the device; enqueued on `stream`, no synchronisation."""
        check(self._fn("search_device")(self._h, C.c_void_p(q_ptr), int(nq), int(k), C.c_void_p(allow_ptr), C.c_void_p(idx_ptr),
                                         C.c_void_p(dist_ptr), C.c_void_p(stream)))

    def get_codes(self, row0=0, nrows=None):
        nrows = self.n - row0 if nrows is None else int(nrows)
        out = np.empty((nrows, self.m), dtype=self._CODE)
        with self._lock:
            check(self._fn("get_codes")(self._h, int(row0), nrows, out.ctypes.data_as(C.c_void_p)))
        return out

    def decode(self, row0=0, nrows=None):
        """-> float32 [nrows, d]: the rows reconstructed from their codes, codebooks[j][code[:, j]] side by side (nanopq's
        pq.decode; mi_pq_decode)."""
        nrows = self.n - row0 if nrows is None else int(nrows)
        out = np.empty((nrows, self.d), dtype=np.float32)
        with self._lock:
            check(self._fn("decode")(self._h, int(row0), nrows, out.ctypes.data_as(C.c_void_p)))
        return out


class PQIndex(_PQBase):
    """PQ index on one MI355X (a `mi_pq` handle): exact ADC top-k on product-quantized codes by (distance asc, id asc)."""
    _DESTROY, _PREFIX, _CODE, _MAX_WORDS, _TRAIN = "mi_pq_destroy", "mi_pq", np.uint8, PQ_MAX_WORDS, staticmethod(pq_train)
    hbm_bytes = _hbm_bytes("mi_pq_info", 7)

    def remove(self, rows):
        """Removes rows in place (mi_pq_remove_rows; faiss IndexPQ.remove_ids): `rows` is anything allow_bitmap takes -- a bool
        mask [n] over the shard's rows, an array of GLOBAL ids (duplicates are fine), or packed AllowBits words.  The survivors
        keep their order and their code bytes and are renumbered from row_offset on; the capacity stays.  -> kept int64 [n']:
        kept[j] is the old global id of new row j.  Raises ValueError, before the library is called, on an id outside
        [row_offset, row_offset + n)."""
        return _remove_rows(self, "mi_pq_remove_rows", rows)


class WidePQIndex(_PQBase):
    """Wide PQ index on one MI355X (a `mi_pqw` handle): PQIndex with 2 <= Ks <= PQW_MAX_WORDS = 8192 codewords
    per book and uint16 codes -- the reference's 16 x 8192 PQ.  The same contract word for word; for Ks <= 256 every output equals
    PQIndex's bit for bit.  No row removal."""
    _DESTROY, _PREFIX, _CODE, _MAX_WORDS, _TRAIN = "mi_pqw_destroy", "mi_pqw", np.uint16, PQW_MAX_WORDS, staticmethod(pqw_train)
    hbm_bytes = _hbm_bytes("mi_pqw_info", 7)


PQ_GRAPH_MAX_SHORTLIST = 2048     # a graph search returns at most ef <= 2048 rows: the longest shortlist refine= can ask for


class PQGraphIndex(_GraphBase):
    """A neighbour graph over the codes of a PQIndex (a `mi_pq_graph` handle): best-first search from a set of
    entry rows on ADC distances, the role of the reference's PQ + HNSW matchers.  No raw rows are resident.  Which rows the graph
    reaches is approximate; the answer given graph, entry rows, codebooks, codes and query is exact: a row's distance has the bits
    it has in PQIndex.search, the order is (distance asc, id asc).  The PQIndex must outlive the graph and is not changed by it;
    after pq.add / pq.append_codes / pq.remove a search raises (build a new graph).  build: GraphIndex.build's table over ADC
    distances -- row i's query is its own reconstruction -- from the exhaustive search of the PQ index; from_neighbors takes
    GraphIndex.neighbors of a graph over the raw rows, for one."""

    _PREFIX, _OWNER, _INFO_EXTRA, _DESTROY = "mi_pq_graph", "pq", (None,), "mi_pq_graph_destroy"
    # table, entries and the grow-only workspace of the searches (the PQ index counts its own)
    hbm_bytes = _hbm_bytes("mi_pq_graph_info", 3)

    def search(self, q, k, ef=None, return_visited=False, refine=None, k_factor=1):
        """-> (ids int64 [Q, k], dist float32 [Q, k], seconds); ef (the size of the candidate list W) defaults to max(k, 64),
        1 <= k <= ef <= 2048.  Fewer than k rows reached: ids -1, distances +inf.  return_visited: int32 [Q], the rows evaluated
        per query, appended to the tuple.
        refine=<Gallery of the raw rows>: the graph search takes min(k * k_factor, n, 2048) ids (never fewer than k) on the device
        with ef raised to that number where it is below, the gallery re-ranks them there (Gallery.refine; queries rounded to
        float32) and the distances returned are its exact float32 values."""
        k, ef = _graph_search_shape(k, ef)
        a, code, rs, cs = self.pq._rows(q)
        nq = a.shape[0]
        if refine is not None:
            if return_visited:
                raise ValueError("return_visited is not available with refine")
            kc = min(refine_kc(k, k_factor, self.n), PQ_GRAPH_MAX_SHORTLIST)       # (k <= ef <= 2048: never below k)
            return _search_refined(refine, a, k, kc, _NO_ALLOW, self.pq.device, self._lock, self.search_device, ef=max(ef, kc))
        vis = np.empty(nq, dtype=np.int32)
        out = self._topk(nq, k, (np.float32,), lambda idx, dist, secs: load().mi_pq_graph_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, ef, idx, dist, C.c_void_p(vis.ctypes.data), secs))
        return out + (vis,) if return_visited else out

    def search_device(self, q_ptr, nq, k, idx_ptr, ef=None, dist_ptr=None, visited_ptr=None, stream=None):
        """mi_pq_graph_search_device: q_ptr packed float32 [nq][d] on the device; enqueued on `stream`, no synchronisation."""
        k, ef = _graph_search_shape(k, ef)
        check(load().mi_pq_graph_search_device(self._h, C.c_void_p(q_ptr), int(nq), k, ef, C.c_void_p(idx_ptr), C.c_void_p(dist_ptr),
                                               C.c_void_p(visited_ptr), C.c_void_p(stream)))


IVF_MAX_LISTS = 256


def ivf_coarse(coarse, d):
    """float32 [nlist, d] C-contiguous coarse centroids, checked against what an IVF-PQ index takes: 2 <= nlist <= 256, finite.
    Raises ValueError."""
    g = np.ascontiguousarray(coarse, dtype=np.float32)
    if g.ndim == 3 and g.shape[0] == 1:              # what pq_train(x, 1, nlist) returns
        g = g[0]
    if g.ndim != 2:
        raise ValueError("coarse centroids must be [nlist, d] (got shape %s)" % (g.shape,))
    if not 2 <= g.shape[0] <= IVF_MAX_LISTS:
        raise ValueError("nlist = %d lists, an IVF-PQ index takes 2 .. %d (one byte per row)" % (g.shape[0], IVF_MAX_LISTS))
    if g.shape[1] != d:
        raise ValueError("coarse centroids of %d columns, the codebooks span d = %d" % (g.shape[1], d))
    if not np.isfinite(g).all():
        raise ValueError("coarse centroids must be finite")
    return g


def ivf_list_ids(lists, rows, nlist):
    """uint8 [rows] C-contiguous list ids from any integer array with values in [0, nlist).  Raises ValueError."""
    a = np.asarray(lists)
    if a.ndim != 1 or a.shape[0] != rows:
        raise ValueError("list ids must be [rows = %d] (got shape %s)" % (rows, a.shape))
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("list ids must be an integer array (got %s)" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= nlist):
        raise ValueError("list ids must lie in [0, nlist = %d)" % nlist)
    return np.ascontiguousarray(a, dtype=np.uint8)


class IVFPQIndex(_Handle):
    """IVF index over PQ codes on one MI355X (a `mi_ivfpq` handle): the exact ADC top-k of PQIndex.search over the rows whose
    list is one of a query's probed lists, by (distance asc, id asc).  by_residual=True at creation gives faiss's IndexIVFPQ
    default: a code quantizes double(x) - double(coarse[list]) and a query has one float64-summed table per probed list; the kind
    is fixed for the life of the index.
    Beyond the C handle, and kept on purpose: every index made by from_codes / from_device_ptr / empty / fit (either kind)
    carries `.coarse` [nlist, d] and `.codebooks` [M, Ks, L], float32 copies of the arrays it was created with -- the handle has no
    getter for them, and knn.ANN's callers and the tests need them to restate an answer; and `train()` is the training half of
    fit() as a classmethod of its own, which knn.ANN uses to train on a sample and add all rows."""
    _DESTROY = "mi_ivfpq_destroy"
    hbm_bytes = _hbm_bytes("mi_ivfpq_info", 8)

    def __init__(self, handle):
        super().__init__(handle)
        self._info()
        kind = C.c_int32()
        check(load().mi_ivfpq_is_residual(self._h, C.byref(kind)))
        self._residual = bool(kind.value)

    @property
    def by_residual(self):
        return self._residual

    def _info(self):
        n, cap, off, hb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        d, m, ks, nlist, dev = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(load().mi_ivfpq_info(self._h, n, d, m, ks, nlist, dev, off, cap, hb))
        self.n, self.d, self.m, self.ks, self.nlist, self.device = n.value, d.value, m.value, ks.value, nlist.value, dev.value
        self.row_offset, self.capacity = off.value, cap.value
        return hb.value

    @classmethod
    def _create(cls, g, cb, codes_ptr, lists_ptr, n, stride, memspace, device, row_offset, capacity, by_residual=False):
        m, ks, L = cb.shape
        h = C.c_void_p()
        create = load().mi_ivfpq_create_residual if by_residual else load().mi_ivfpq_create
        check(create(C.c_void_p(g.ctypes.data), g.shape[0], C.c_void_p(cb.ctypes.data), m * L, m, ks, C.c_void_p(codes_ptr),
                     C.c_void_p(lists_ptr), int(n), int(stride), memspace, device, int(row_offset), int(capacity), C.byref(h)))
        idx = cls(h.value)
        idx.coarse, idx.codebooks = g.copy(), cb.copy()
        return idx

    @classmethod
    def from_codes(cls, coarse, codebooks, codes, lists, device=0, row_offset=0, capacity=0, by_residual=False):
        """coarse [nlist, d] float32, codebooks [M, Ks, L] float32, codes integer [N, M] in [0, Ks), lists integer [N] in
        [0, nlist); capacity 0 = N, larger leaves room for append_codes() / add().  by_residual=True: the codes are residual codes."""
        cb = pq_codebooks(codebooks)
        g = ivf_coarse(coarse, cb.shape[0] * cb.shape[2])
        a, stride = pq_code_rows(codes, cb.shape[0], cb.shape[1])
        li = ivf_list_ids(lists, a.shape[0], g.shape[0])
        if capacity and capacity < a.shape[0]:
            raise ValueError("capacity %d below the %d rows given" % (capacity, a.shape[0]))
        return cls._create(g, cb, a.ctypes.data, li.ctypes.data, a.shape[0], stride, MI_HOST, device, row_offset, capacity, by_residual)

    @classmethod
    def from_device_ptr(cls, coarse, codebooks, codes_ptr, lists_ptr, n, device=0, row_offset=0, capacity=0, row_stride_bytes=None,
                        by_residual=False):
        """Device codes [n][M] uint8 and list ids [n] uint8 -> index, synchronous; their producer must have completed."""
        cb = pq_codebooks(codebooks)
        g = ivf_coarse(coarse, cb.shape[0] * cb.shape[2])
        return cls._create(g, cb, codes_ptr, lists_ptr, n, cb.shape[0] if row_stride_bytes is None else row_stride_bytes, MI_DEVICE,
                           device, row_offset, capacity, by_residual)

    @classmethod
    def empty(cls, coarse, codebooks, capacity, device=0, row_offset=0, by_residual=False):
        """Appendable index: `capacity` rows allocated, filled by append_codes() / add()."""
        cb = pq_codebooks(codebooks)
        g = ivf_coarse(coarse, cb.shape[0] * cb.shape[2])
        if int(capacity) < 1:
            raise ValueError("an empty index needs a capacity")
        return cls._create(g, cb, None, None, 0, cb.shape[0], MI_HOST, device, row_offset, capacity, by_residual)

    @classmethod
    def train(cls, x, nlist, M, Ks, iters=20, seed=42, device=0, by_residual=False):
        """The training of fit() without the index: -> (coarse float32 [nlist, d], codebooks float32 [M, Ks, L], coarse_moved,
        train_moved).  The coarse centroids are pq_train with ONE book of nlist codewords.  by_residual=False: the codebooks are
        pq_train on x.  by_residual=True: the rows are assigned to their lists, the float32 residual rows
        float32(double(x) - double(coarse[list])) are formed on the device and pq_train_device runs on them, with the seed rule
        of pq_train (initial rows drawn by RandomState(seed), taken from the residual rows; seed=None: the library's default)."""
        nlist = int(nlist)
        if not 2 <= nlist <= IVF_MAX_LISTS:
            raise ValueError("nlist = %d lists, an IVF-PQ index takes 2 .. %d (one byte per row)" % (nlist, IVF_MAX_LISTS))
        if by_residual:                                  # the limits of the second training, before the first touches the device
            n, d = np.shape(x)
            M, Ks, iters = int(M), int(Ks), int(iters)
            L = _pq_train_shape(n, d, M, Ks, iters)
        g, gmoved = pq_train(x, 1, nlist, iters=iters, seed=seed, device=device)
        if not by_residual:
            cb, moved = pq_train(x, M, Ks, iters=iters, seed=seed, device=device)
            return g[0], cb, gmoved, moved
        import torch
        res = torch.empty((n, d), dtype=torch.float32, device="cuda:%d" % device)
        with cls.empty(g[0], np.zeros((M, Ks, L), np.float32), 1, device=device) as tmp:      # the centroids are all it is used for
            tmp.residual_rows_device(x, res.data_ptr())
        cb0 = None
        if seed is not None:
            rng = np.random.RandomState(seed)
            rows = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
            picked = res[torch.as_tensor(rows.reshape(-1), device=res.device)].cpu().numpy().reshape(M, Ks, d)
            cb0 = np.ascontiguousarray(np.stack([picked[j, :, j * L:(j + 1) * L] for j in range(M)]), dtype=np.float32)
        cb, moved = pq_train_device(res.data_ptr(), n, d, M, Ks, iters, init=cb0, device=device)
        return g[0], cb, gmoved, moved

    @classmethod
    def fit(cls, x, nlist, M, Ks, iters=20, seed=42, capacity=0, device=0, row_offset=0, by_residual=False):
        """Learns the coarse centroids (pq_train with ONE book of nlist codewords) and the codebooks (pq_train) on x [n, d], both
        with `seed`, creates the index and adds x.  by_residual=True: the codebooks are learned on the residual rows (train()) and
        the index is a residual index.  The move counts are in `.coarse_moved` and `.train_moved`."""
        nlist = int(nlist)
        if not 2 <= nlist <= IVF_MAX_LISTS:
            raise ValueError("nlist = %d lists, an IVF-PQ index takes 2 .. %d (one byte per row)" % (nlist, IVF_MAX_LISTS))
        n = np.shape(x)[0]
        if capacity and capacity < n:
            raise ValueError("capacity %d below the %d rows given" % (capacity, n))
        g, cb, gmoved, moved = cls.train(x, nlist, M, Ks, iters=iters, seed=seed, device=device, by_residual=by_residual)
        idx = cls.empty(g, cb, capacity or n, device=device, row_offset=row_offset, by_residual=by_residual)
        idx.coarse_moved, idx.train_moved = gmoved, moved
        idx.add(x)
        return idx

    def _rows(self, x):
        a, code, rs, cs = _strided(x)
        if a.shape[1] != self.d:
            raise ValueError("rows of %d columns, the index takes %d" % (a.shape[1], self.d))
        return a, code, rs, cs

    def _nprobe(self, nprobe):
        nprobe = int(nprobe)
        if not 1 <= nprobe <= self.nlist:
            raise ValueError("nprobe = %d, the index has nlist = %d lists (1 .. nlist)" % (nprobe, self.nlist))
        return nprobe

    def append_codes(self, codes, lists):
        a, stride = pq_code_rows(codes, self.m, self.ks)
        li = ivf_list_ids(lists, a.shape[0], self.nlist)
        with self._lock:
            check(load().mi_ivfpq_append_codes(self._h, C.c_void_p(a.ctypes.data), C.c_void_p(li.ctypes.data), a.shape[0], stride, MI_HOST))
            self.n += a.shape[0]

    def append_codes_device(self, codes_ptr, lists_ptr, rows, row_stride_bytes=None):
        with self._lock:
            check(load().mi_ivfpq_append_codes(self._h, C.c_void_p(codes_ptr), C.c_void_p(lists_ptr), int(rows),
                                               self.m if row_stride_bytes is None else int(row_stride_bytes), MI_DEVICE))
            self.n += int(rows)

    def add(self, x):
        """Assigns rows [rows, d] float32/float64 (any strides) to their lists, encodes them on the device and appends."""
        a, code, rs, cs = self._rows(x)
        with self._lock:
            check(load().mi_ivfpq_add(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST))
            self.n += a.shape[0]

    def add_device(self, x_ptr, rows, dtype=MI_F32, row_stride=None, col_stride=1):
        with self._lock:
            check(load().mi_ivfpq_add(self._h, C.c_void_p(x_ptr), int(rows), dtype, self.d if row_stride is None else int(row_stride),
                                      int(col_stride), MI_DEVICE))
            self.n += int(rows)

    def _lists(self, lists, rows):
        return None if lists is None else ivf_list_ids(lists, rows, self.nlist)

    def residual_rows(self, x, lists=None):
        """-> float32 [rows, d]: float32(double(x) - double(coarse[l])), one rounding, computed on the device; l is lists[row]
        (integer [rows] in [0, nlist)) or, with lists None, the list the index assigns.  Either kind of index; it is unchanged."""
        a, code, rs, cs = self._rows(x)
        li = self._lists(lists, a.shape[0])
        out = np.empty((a.shape[0], self.d), dtype=np.float32)
        with self._lock:
            check(load().mi_ivfpq_residual_rows(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST,
                                                None if li is None else C.c_void_p(li.ctypes.data), out.ctypes.data_as(C.c_void_p),
                                                MI_HOST))
        return out

    def residual_rows_device(self, x, out_ptr, lists=None):
        """residual_rows of host rows into a device buffer float32 [rows][d] at out_ptr; synchronous."""
        a, code, rs, cs = self._rows(x)
        li = self._lists(lists, a.shape[0])
        with self._lock:
            check(load().mi_ivfpq_residual_rows(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, MI_HOST,
                                                None if li is None else C.c_void_p(li.ctypes.data), C.c_void_p(int(out_ptr)), MI_DEVICE))

    def probe(self, q, nprobe=1):
        """-> int32 [Q, nprobe]: per query the nprobe lists nearest in float64, nearest first, ties to the lower list."""
        a, code, rs, cs = self._rows(q)
        nprobe = self._nprobe(nprobe)
        out = np.empty((a.shape[0], nprobe), dtype=np.int32)
        with self._lock:
            check(load().mi_ivfpq_probe(self._h, C.c_void_p(_base_pointer(a)), a.shape[0], code, rs, cs, nprobe,
                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def search(self, q, k, nprobe=1, probes=None, allow=None, allow_ptr=None, refine=None, k_factor=1):
        """-> (ids int64 [Q,k], dist float32 [Q,k], seconds), ordered by (distance asc, id asc), over the rows of the probed
        lists.  probes: integer [Q, P] of list ids, -1 = no list, repeats ignored (then nprobe is P); None: the library probes the
        nprobe nearest lists.  allow / allow_ptr as for PQIndex.search.  Fewer than k such rows: trailing ids -1, distances +inf.
        refine=<Gallery of the raw rows>: the search takes refine_kc(k, k_factor, n) ids on the device, the gallery re-ranks them
        there (Gallery.refine; queries rounded to float32) and the distances returned are its exact float32 values."""
        a, code, rs, cs = self._rows(q)
        nq, k = a.shape[0], int(k)
        resolved = bits, bits_p, memspace = _resolve_allow(allow, allow_ptr, self.n, self.row_offset)
        pr, pr_p = None, None
        if probes is not None:
            pr = np.asarray(probes)
            if pr.ndim != 2 or pr.shape[0] != nq or pr.dtype == np.bool_ or not np.issubdtype(pr.dtype, np.integer):
                raise ValueError("probes must be an integer array [Q = %d, P] (got %s %s)" % (nq, pr.dtype, pr.shape))
            if pr.size and (int(pr.min()) < -1 or int(pr.max()) >= self.nlist):
                raise ValueError("probes must be -1 or lie in [0, nlist = %d)" % self.nlist)
            nprobe = pr.shape[1]
            pr = np.ascontiguousarray(pr, dtype=np.int32)
            pr_p = C.c_void_p(pr.ctypes.data)
        nprobe = self._nprobe(nprobe)
        if refine is not None:
            import torch

            def stage(xq, stream):
                return xq, {"probes_ptr": torch.from_numpy(pr).to(xq.device)}
            return _search_refined(refine, a, k, refine_kc(k, k_factor, self.n), resolved, self.device, self._lock, self.search_device,
                                   stage=None if pr is None else stage, nprobe=nprobe)
        return self._topk(nq, k, (np.float32,), lambda idx, dist, secs: load().mi_ivfpq_search(
            self._h, C.c_void_p(_base_pointer(a)), nq, code, rs, cs, k, nprobe, pr_p, bits_p, memspace, idx, dist, secs))

    def search_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, nprobe=1, probes_ptr=None, allow_ptr=None, stream=None):
        """q_ptr: packed float32 [nq][d] on the device; probes_ptr: None or int32 [nq][nprobe] on the device (entries outside
        [0, nlist) count as -1); enqueued on `stream`, no synchronisation."""
        check(load().mi_ivfpq_search_device(self._h, C.c_void_p(q_ptr), int(nq), int(k), int(nprobe), C.c_void_p(probes_ptr),
                                            C.c_void_p(allow_ptr), C.c_void_p(idx_ptr), C.c_void_p(dist_ptr), C.c_void_p(stream)))

    def search_stages_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, nprobe=1, stream=None):
        """search_device with the library's probes, measured: -> (table_ms, scan_ms), HIP-event times of the table kernel and of the
        scan-and-select summed over the chunks of the batch.  Synchronous; for benchmarks."""
        t, u = C.c_float(), C.c_float()
        check(load().mi_ivfpq_search_stages_device(self._h, C.c_void_p(q_ptr), int(nq), int(k), int(nprobe), C.c_void_p(idx_ptr),
                                                   C.c_void_p(dist_ptr), C.c_void_p(stream), C.byref(t), C.byref(u)))
        return t.value, u.value

    def list_sizes(self):
        out = np.empty(self.nlist, dtype=np.int64)
        check(load().mi_ivfpq_list_sizes(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def remove(self, rows):
        """Removes rows in place (mi_ivfpq_remove_rows; faiss IndexIVFPQ.remove_ids), either kind of index: arguments, return
        value and errors of PQIndex.remove.  A survivor stays in its list; the blocks the lists no longer reach are reused by
        later appends."""
        return _remove_rows(self, "mi_ivfpq_remove_rows", rows)

    def get_rows(self, row0=0, nrows=None):
        """-> (codes uint8 [nrows, M], lists uint8 [nrows]) of the rows row0 .. row0 + nrows in the order they were given."""
        nrows = self.n - row0 if nrows is None else int(nrows)
        codes = np.empty((nrows, self.m), dtype=np.uint8)
        lists = np.empty(nrows, dtype=np.uint8)
        with self._lock:
            check(load().mi_ivfpq_get_rows(self._h, int(row0), nrows, codes.ctypes.data_as(C.c_void_p), lists.ctypes.data_as(C.c_void_p)))
        return codes, lists


IVFFLAT_MAX_LISTS = 8192          # lists of an IVFFlatIndex (mi_ivfflat)
IVFFLAT_MAX_K = 2048
IVFFLAT_SLAB_ROWS = 2048          # positions of a query's candidate sequence one scan workgroup sorts (csrc/kernels.h)


def ivfflat_centroids(centroids, d):
    """float32 [nlist, d] C-contiguous centroids, checked against what an IVF-Flat index takes: 2 <= nlist <= 8192, finite.  Raises
    ValueError."""
    g = np.asarray(centroids)
    if g.ndim == 3 and g.shape[0] == 1:              # what pq_train(x, 1, nlist) returns
        g = g[0]
    if g.ndim != 2 or g.dtype == np.bool_ or not (np.issubdtype(g.dtype, np.floating) or np.issubdtype(g.dtype, np.integer)):
        raise ValueError("centroids must be a numeric array [nlist, d] (got %s %s)" % (g.dtype, g.shape))
    if not 2 <= g.shape[0] <= IVFFLAT_MAX_LISTS:
        raise ValueError("nlist = %d lists, an IVF-Flat index takes 2 .. %d" % (g.shape[0], IVFFLAT_MAX_LISTS))
    if g.shape[1] != int(d):
        raise ValueError("centroids of %d columns, the gallery has d = %d" % (g.shape[1], d))
    g = np.ascontiguousarray(g, dtype=np.float32)
    if not np.isfinite(g).all():
        raise ValueError("centroids must be finite")
    return g


def ivfflat_list_ids(list_ids, n, nlist):
    """int32 [n] C-contiguous list ids from any integer array with values in [0, nlist).  Raises ValueError."""
    a = np.asarray(list_ids)
    if a.ndim != 1 or a.shape[0] != int(n):
        raise ValueError("list ids must be [n = %d] (got shape %s)" % (n, a.shape))
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("list ids must be an integer array (got %s)" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= nlist):
        raise ValueError("list ids must lie in [0, nlist = %d)" % nlist)
    return np.ascontiguousarray(a, dtype=np.int32)


def _ivfflat_rows(n):
    n = int(n)
    if n < 1 or n >= 2 ** 31:
        raise ValueError("an IVF-Flat index takes a gallery of 1 .. 2^31 - 1 rows (got %d)" % n)
    return n


class IVFFlatIndex(_Handle):
    """An inverted file over the raw rows of a Gallery (a `mi_ivfflat` handle), faiss IndexIVFFlat: every row
    belongs to the list of its best centroid, a query evaluates the stored rows of the nprobe lists it probes.  Which rows are
    reached is approximate; the answer given centroids, lists, stored rows and query is exact: values are Gallery.refine's, the
    order is (value best first, id ascending).  The rows are not copied: the index costs 4 bytes per row plus the centroids.  The
    gallery must outlive the index.  The index follows its gallery in place: after gallery.append* call sync(), and remove rows
    through remove() of the index, which removes them from the gallery too; either leaves the lists and answers of a fresh
    build(gallery, the same centroids), bit for bit.  Until sync() an appended-to gallery makes probe and search raise, and a
    gallery.remove() made beside the index makes probe, search and sync() raise for good (build a new index).  Nothing routes to
    this index by default and its speed has not been measured: for large batches the exhaustive search stays the choice."""
    _DESTROY = "mi_ivfflat_destroy"
    hbm_bytes = _hbm_bytes("mi_ivfflat_info", 3)

    def __init__(self, handle, gallery):
        super().__init__(handle)
        self.gallery = gallery
        n, d, nlist = C.c_int64(), C.c_int32(), C.c_int32()
        check(load().mi_ivfflat_info(self._h, n, d, nlist, None))
        self.n, self.d, self.nlist = n.value, d.value, nlist.value

    @staticmethod
    def train(x, nlist, iters=20, seed=0, device=0):
        """-> centroids float32 [nlist, d]: deterministic k-means on x [n, d] with ONE book of nlist full-dimension codewords,
        pq_train up to 256 lists and pqw_train above that (up to 8192).  train_matrix returns the same centroids bit for bit with
        the assignment at f64 matrix rate."""
        nlist = int(nlist)
        if not 2 <= nlist <= IVFFLAT_MAX_LISTS:
            raise ValueError("nlist = %d lists, an IVF-Flat index takes 2 .. %d" % (nlist, IVFFLAT_MAX_LISTS))
        fit = pq_train if nlist <= PQ_MAX_WORDS else pqw_train
        return np.ascontiguousarray(fit(x, 1, nlist, iters=iters, seed=seed, device=device)[0][0], dtype=np.float32)

    @staticmethod
    def train_matrix(x, nlist, iters=20, seed=0, device=0):
        """train with the assignment at f64 matrix rate (kmeans_train): the same arguments, the same centroids bit for bit."""
        nlist = int(nlist)
        if not 2 <= nlist <= IVFFLAT_MAX_LISTS:
            raise ValueError("nlist = %d lists, an IVF-Flat index takes 2 .. %d" % (nlist, IVFFLAT_MAX_LISTS))
        return kmeans_train(x, nlist, iters=iters, seed=seed, device=device)[0]

    @classmethod
    def build(cls, gallery, centroids):
        """mi_ivfflat_build: every stored row of `gallery` goes to the list of its best centroid (centroids float [nlist, d]), on
        the device.  Deterministic.  Bad shapes raise ValueError before the device is touched."""
        _ivfflat_rows(gallery.n)
        g = ivfflat_centroids(centroids, gallery.d)
        h = C.c_void_p()
        with gallery._lock:
            check(load().mi_ivfflat_build(gallery._h, C.c_void_p(g.ctypes.data), g.shape[0], C.byref(h)))
        return cls(h.value, gallery)

    @classmethod
    def from_lists(cls, gallery, centroids, list_ids):
        """mi_ivfflat_create: list_ids integer [n] in [0, nlist), the list of every row.  Bad input raises ValueError before the
        device is touched."""
        n = _ivfflat_rows(gallery.n)
        g = ivfflat_centroids(centroids, gallery.d)
        li = ivfflat_list_ids(list_ids, n, g.shape[0])
        h = C.c_void_p()
        with gallery._lock:
            check(load().mi_ivfflat_create(gallery._h, C.c_void_p(g.ctypes.data), g.shape[0], C.c_void_p(li.ctypes.data), MI_HOST,
                                           C.byref(h)))
        return cls(h.value, gallery)

    def _nprobe(self, nprobe):
        nprobe = int(nprobe)
        if not 1 <= nprobe <= self.nlist:
            raise ValueError("nprobe = %d, the index has nlist = %d lists (1 .. nlist)" % (nprobe, self.nlist))
        return nprobe

    def _k(self, k):
        k = int(k)
        if not 1 <= k <= IVFFLAT_MAX_K:
            raise ValueError("k = %d: k must be in [1, %d]" % (k, IVFFLAT_MAX_K))
        return k

    def _stage(self, q):
        """Host queries [Q, d] of any float type and strides -> (packed float32 tensor on the gallery's device, torch device, stream):
        float64 is rounded to float32, as the host entry points of the library do."""
        import torch
        a = self.gallery._queries(q)[0]
        tdev = "cuda:%d" % self.gallery.device
        xq = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(tdev)
        return xq, tdev, torch.cuda.current_stream(tdev).cuda_stream

    def probe(self, q, nprobe=1):
        """-> int32 [Q, nprobe]: per query its nprobe best lists, best first, ties to the lower list (mi_ivfflat_probe_device on the
        staged queries; synchronous)."""
        import torch
        nprobe = self._nprobe(nprobe)
        xq, tdev, stream = self._stage(q)
        nq = xq.shape[0]
        if nq == 0:
            return np.empty((0, nprobe), np.int32)
        out = torch.empty((nq, nprobe), dtype=torch.int32, device=tdev)
        with self._lock:
            self.probe_device(xq.data_ptr(), nq, nprobe, out.data_ptr(), stream=stream)
            return out.cpu().numpy()                       # (synchronises with the stream the work is on)

    def probe_device(self, q_ptr, nq, nprobe, out_ptr, stream=None):
        """mi_ivfflat_probe_device: q_ptr packed float32 [nq][d], out_ptr int32 [nq][nprobe] on the device; enqueued on `stream`."""
        check(load().mi_ivfflat_probe_device(self._h, C.c_void_p(q_ptr), int(nq), self._nprobe(nprobe), C.c_void_p(out_ptr),
                                             C.c_void_p(stream)))

    def search(self, q, k, nprobe=1, probes=None, allow=None, return_values64=False, return_scanned=False):
        """-> (ids int64 [Q, k], values float32 [Q, k], seconds), 1 <= k <= 2048, over the rows of the probed lists, by (value best
        first, id ascending).  probes: integer [Q, P] of list ids in place of the library's nprobe best lists (then nprobe is P); an
        entry outside [0, nlist) or repeating an earlier one of its row is no list.  allow: anything allow_bitmap takes.  Fewer than
        k such rows: ids -1, values +inf (L2) / -inf.  return_values64: the float64 values in place of their float32 cast;
        return_scanned: a fourth result, int64 [Q], the rows evaluated per query.  The queries, the probes and the bitmap are
        staged on the device here and mi_ivfflat_search_device does the work; seconds is the wall time of that, staging and the
        copies back included; synchronous."""
        import torch
        k = self._k(k)
        a = self.gallery._queries(q)[0]
        nq = a.shape[0]
        bits = _allow_words(allow, self.n, self.gallery.row_offset)
        pr = None
        if probes is not None:
            pr = np.asarray(probes)
            if pr.ndim != 2 or pr.shape[0] != nq or pr.dtype == np.bool_ or not np.issubdtype(pr.dtype, np.integer):
                raise ValueError("probes must be an integer array [Q = %d, P] (got %s %s)" % (nq, pr.dtype, pr.shape))
            nprobe = pr.shape[1]
            pr = np.ascontiguousarray(np.where((pr < 0) | (pr >= self.nlist), -1, pr), dtype=np.int32)
        nprobe = self._nprobe(nprobe)
        if nq == 0:
            out = (np.empty((0, k), np.int64), np.empty((0, k), np.float64 if return_values64 else np.float32), 0.0)
            return (*out, np.empty(0, np.int64)) if return_scanned else out
        t0 = time.perf_counter()
        xq, tdev, stream = self._stage(a)
        bits_dev = _upload_allow(bits, tdev)
        pr_dev = None if pr is None else torch.from_numpy(pr).to(tdev)
        idx = torch.empty((nq, k), dtype=torch.int64, device=tdev)
        val = torch.empty((nq, k), dtype=torch.float32, device=tdev)
        val64 = torch.empty((nq, k), dtype=torch.float64, device=tdev)
        scanned = torch.empty((nq,), dtype=torch.int64, device=tdev)
        with self._lock:
            self.search_device(xq.data_ptr(), nq, k, idx.data_ptr(), val_ptr=val.data_ptr(), val64_ptr=val64.data_ptr(), nprobe=nprobe,
                               probes_ptr=None if pr_dev is None else pr_dev.data_ptr(),
                               allow_ptr=None if bits_dev is None else bits_dev.data_ptr(), scanned_ptr=scanned.data_ptr(), stream=stream)
            ids, vv = idx.cpu().numpy(), (val64 if return_values64 else val).cpu().numpy()      # (synchronises with the stream)
            sc = scanned.cpu().numpy()
        out = (ids, vv, time.perf_counter() - t0)
        return (*out, sc) if return_scanned else out

    def search_device(self, q_ptr, nq, k, idx_ptr, val_ptr=None, val64_ptr=None, nprobe=1, probes_ptr=None, allow_ptr=None,
                      scanned_ptr=None, stream=None):
        """mi_ivfflat_search_device: q_ptr packed float32 [nq][d] on the device; probes_ptr: None or int32 [nq][nprobe] on the
        device; allow_ptr: None or the bitmap on the device; enqueued on `stream`, no synchronisation."""
        check(load().mi_ivfflat_search_device(self._h, C.c_void_p(q_ptr), int(nq), self._k(k), self._nprobe(nprobe), C.c_void_p(probes_ptr),
                                              C.c_void_p(allow_ptr), C.c_void_p(idx_ptr), C.c_void_p(val_ptr), C.c_void_p(val64_ptr),
                                              C.c_void_p(scanned_ptr), C.c_void_p(stream)))

    def sync(self):
        """mi_ivfflat_sync: takes in the rows appended to the gallery since the index was made or last updated -> their number.
        Afterwards the index is the one build() makes on the gallery as it stands.  Raises RuntimeError after a gallery.remove()
        made beside the index."""
        added = C.c_int64()
        with self.gallery._lock, self._lock:
            check(load().mi_ivfflat_sync(self._h, C.byref(added)))
            self.n += added.value
        return added.value

    def remove(self, rows):
        """mi_ivfflat_remove_rows: removes rows from the gallery AND from the index -> their number.  `rows` is anything
        Gallery.remove takes (a bool mask [n], an array of GLOBAL ids, packed AllowBits words); the survivors are renumbered as
        Gallery.remove renumbers them, and gallery.n follows.  Afterwards the index is the one build() makes on the gallery as it
        stands.  Raises ValueError, before the library is called, on a bad `rows`; RuntimeError when every row is named, when the
        index is not in step with its gallery, and whenever Gallery.remove would."""
        g = self.gallery
        bits = allow_bitmap(rows, g.n, g.row_offset)
        removed = C.c_int64()
        with g._lock, self._lock:
            check(load().mi_ivfflat_remove_rows(self._h, C.c_void_p(bits.ctypes.data), MI_HOST, C.byref(removed)))
            g.n -= removed.value
            self.n -= removed.value
        return removed.value

    def list_sizes(self):
        """-> int64 [nlist]: the rows of every list."""
        out = np.empty(self.nlist, dtype=np.int64)
        check(load().mi_ivfflat_list_sizes(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def lists(self):
        """-> (list_off int64 [nlist + 1], list_rows int32 [n]): list l holds the local rows list_rows[list_off[l]:list_off[l + 1]],
        ascending."""
        off, rows = np.empty(self.nlist + 1, np.int64), np.empty(self.n, np.int32)
        with self._lock:
            check(load().mi_ivfflat_get_lists(self._h, C.c_void_p(off.ctypes.data), C.c_void_p(rows.ctypes.data)))
        return off, rows

    def list_ids(self):
        """-> int32 [n]: the list of every row, read back from lists()."""
        off, rows = self.lists()
        out = np.empty(self.n, np.int32)
        out[rows] = np.repeat(np.arange(self.nlist, dtype=np.int32), np.diff(off))
        return out

    def centroids(self):
        """-> float32 [nlist, d]."""
        out = np.empty((self.nlist, self.d), np.float32)
        with self._lock:
            check(load().mi_ivfflat_get_centroids(self._h, C.c_void_p(out.ctypes.data)))
        return out


def kth_of_gathered_device(gathered_ptr, nshards, nq, k, out_ptr, stream=None):
    check(load().mi_kth_of_gathered_device(C.c_void_p(gathered_ptr), nshards, nq, k, C.c_void_p(out_ptr),
                                           C.c_void_p(stream)))


def topk_merge_strided_device(score64_ptr, idx_ptr, shard_stride, nshards, nq, k, out_idx_ptr, out_score_ptr, stream=None):
    check(load().mi_topk_merge_strided_device(C.c_void_p(score64_ptr), C.c_void_p(idx_ptr), shard_stride, nshards, nq, k,
                                              C.c_void_p(out_idx_ptr), C.c_void_p(out_score_ptr), C.c_void_p(stream)))


def topk_merge_device(score64_ptr, idx_ptr, nshards, nq, k, out_idx_ptr, out_score_ptr, stream=None):
    check(load().mi_topk_merge_device(C.c_void_p(score64_ptr), C.c_void_p(idx_ptr), nshards, nq, k,
                                      C.c_void_p(out_idx_ptr), C.c_void_p(out_score_ptr), C.c_void_p(stream)))


def aqe_combine_device(rows_ptr, nq, d, k_qe, w, sum_ptr, stream=None):
    check(load().mi_aqe_combine_device(C.c_void_p(rows_ptr), nq, d, k_qe, float(w), C.c_void_p(sum_ptr), C.c_void_p(stream)))


def aqe_finish_device(sum_ptr, nq, d, eps, out_q_ptr, out_q64_ptr=None, stream=None):
    check(load().mi_aqe_finish_device(C.c_void_p(sum_ptr), nq, d, float(eps), C.c_void_p(out_q_ptr),
                                      C.c_void_p(out_q64_ptr), C.c_void_p(stream)))


def synth_fill_device(dst_ptr, seed, row0, nrows, d, stream=None):
    check(load().mi_synth_fill_device(C.c_void_p(dst_ptr), seed, row0, nrows, d, C.c_void_p(stream)))


def column_sum(rows, device=0):
    """float64 column sums of a 2-D float array (any strides), computed on the device."""
    a, code, rs, cs = _strided(rows)
    out = np.empty(a.shape[1], dtype=np.float64)
    check(load().mi_column_sum(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs, device,
                               out.ctypes.data_as(C.c_void_p)))
    return out


def column_sum_device(x_ptr, n, d, out_ptr, dtype=MI_F32, row_stride=None, col_stride=1, stream=None):
    """Device twin of column_sum (no synchronisation): out f64 [d]."""
    check(load().mi_column_sum_device(C.c_void_p(x_ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride,
                                      C.c_void_p(out_ptr), C.c_void_p(stream)))


def scatter_workspace_bytes(d):
    """Bytes of device workspace scatter_matrix_device needs for dimension d."""
    b = C.c_int64()
    check(load().mi_scatter_workspace_bytes(int(d), C.byref(b)))
    return b.value


def scatter_matrix(rows, centre=None, pairs=None, device=0):
    """rows [N, D] host array (any strides; f32 | f64) -> float64 [D, D]: sum_n (x_n - centre)(x_n - centre)^T, or with
    pairs = (q, p) index arrays sum_i (x_q_i - x_p_i)(x_q_i - x_p_i)^T.  X moves in row blocks, never whole."""
    a, code, rs, cs = _strided(rows)
    n, d = a.shape
    c = None if centre is None else np.ascontiguousarray(np.asarray(centre, dtype=np.float64).reshape(-1))
    if c is not None and c.shape[0] != d:
        raise ValueError("centre has %d entries for %d columns" % (c.shape[0], d))
    q = p = None
    if pairs is not None:
        q = np.ascontiguousarray(np.asarray(pairs[0]).reshape(-1), dtype=np.int64)
        p = np.ascontiguousarray(np.asarray(pairs[1]).reshape(-1), dtype=np.int64)
        if q.shape != p.shape:
            raise ValueError("pairs: %d q indices, %d p indices" % (q.size, p.size))
    out = np.empty((d, d), dtype=np.float64)
    check(load().mi_scatter_matrix(C.c_void_p(_base_pointer(a)), n, d, code, rs, cs,
                                   None if c is None else c.ctypes.data_as(C.c_void_p),
                                   None if q is None else q.ctypes.data_as(C.c_void_p),
                                   None if p is None else p.ctypes.data_as(C.c_void_p), 0 if q is None else q.size,
                                   int(device), out.ctypes.data_as(C.c_void_p)))
    return out


def scatter_matrix_device(x_ptr, n, d, c_out_ptr, workspace_ptr, workspace_bytes, centre_ptr=None, pair_q_ptr=None,
                          pair_p_ptr=None, n_pairs=0, accumulate=False, dtype=MI_F32, row_stride=None, col_stride=1,
                          stream=None):
    """Device-resident scatter matrix (no synchronisation): c_out f64 [d, d]; workspace of scatter_workspace_bytes(d)."""
    check(load().mi_scatter_matrix_device(C.c_void_p(x_ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride,
                                          C.c_void_p(centre_ptr), C.c_void_p(pair_q_ptr), C.c_void_p(pair_p_ptr), n_pairs,
                                          C.c_void_p(c_out_ptr), 1 if accumulate else 0, C.c_void_p(workspace_ptr),
                                          int(workspace_bytes), C.c_void_p(stream)))


def whiten_apply(rows, m, P, dims, eps=1e-6, device=0):
    """rows [N,D] (any strides) -> float64 [N,dims] = rows of P[:dims] (x - m) / (||.|| + eps)."""
    a, code, rs, cs = _strided(rows)
    m = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(-1))
    Pd = np.ascontiguousarray(np.asarray(P, dtype=np.float64)[:dims, :])
    out = np.empty((a.shape[0], dims), dtype=np.float64)
    check(load().mi_whiten_apply(C.c_void_p(_base_pointer(a)), a.shape[0], a.shape[1], code, rs, cs,
                                 m.ctypes.data_as(C.c_void_p), Pd.ctypes.data_as(C.c_void_p), dims, float(eps), device,
                                 out.ctypes.data_as(C.c_void_p)))
    return out


def whiten_apply_device(x_ptr, n, d, m_ptr, p_ptr, dims, out_ptr, eps=1e-6, dtype=MI_F32, row_stride=None, col_stride=1,
                        stream=None):
    """Device-resident whitenapply (no synchronisation): out f64 [n, dims] = rows of P[:dims] (x - m) / (||.|| + eps);
    eps < 0 leaves the rows un-normalised."""
    check(load().mi_whiten_apply_device(C.c_void_p(x_ptr), n, d, dtype, d if row_stride is None else row_stride, col_stride,
                                        C.c_void_p(m_ptr), C.c_void_p(p_ptr), dims, float(eps), C.c_void_p(out_ptr),
                                        C.c_void_p(stream)))


def desc_tail_device(feat_ptr, b, c, hw, p, eps, w_ptr, b_ptr, c_out, scratch_ptr, out_ptr, stream=None):
    check(load().mi_desc_tail_device(C.c_void_p(feat_ptr), b, c, hw, float(p), float(eps), C.c_void_p(w_ptr),
                                     C.c_void_p(b_ptr), c_out, C.c_void_p(scratch_ptr), C.c_void_p(out_ptr),
                                     C.c_void_p(stream)))


def desc_ms_accumulate_device(acc_ptr, desc_ptr, count, msp, first, stream=None):
    check(load().mi_desc_ms_accumulate_device(C.c_void_p(acc_ptr), C.c_void_p(desc_ptr), count, float(msp),
                                              1 if first else 0, C.c_void_p(stream)))


def desc_ms_finish_device(acc_ptr, b, d, nscales, msp, stream=None):
    check(load().mi_desc_ms_finish_device(C.c_void_p(acc_ptr), b, d, nscales, float(msp), C.c_void_p(stream)))


def kr_rerank(queries, gallery, k1=20, k2=6, lambda_value=0.3, device=0, return_dist=False):
    """queries [Q, D], gallery [N, D] (any float strides) -> indices int64 [Q, N][, final distances float32 [Q, N]]."""
    q, code, qrs, qcs = _strided(queries)
    g, gcode, grs, gcs = _strided(gallery)
    if gcode != code:
        g = g.astype(q.dtype)
        g, gcode, grs, gcs = _strided(g)
    if q.shape[1] != g.shape[1]:
        raise ValueError("query dimension %d != gallery dimension %d" % (q.shape[1], g.shape[1]))
    idx = np.empty((q.shape[0], g.shape[0]), dtype=np.int64)
    dist = np.empty((q.shape[0], g.shape[0]), dtype=np.float32) if return_dist else None
    check(load().mi_kr_rerank(C.c_void_p(_base_pointer(q)), q.shape[0], qrs, qcs, C.c_void_p(_base_pointer(g)), g.shape[0],
                              grs, gcs, q.shape[1], code, int(k1), int(k2), float(lambda_value), int(device),
                              idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p) if return_dist else None))
    return (idx, dist) if return_dist else idx


_default_image_f16 = [1]


def set_global_option(name, value):
    if name == "image_dtype":
        _default_image_f16[0] = 1 if value else 0
    check(load().mi_set_global_option(name.encode(), float(value)))


def get_global_option(name):
    """"image_dtype", "host_ingest", "keep_buffers", "spare_bytes" (device memory held in the spare slots right now)."""
    v = C.c_double(0.0)
    check(load().mi_get_global_option(name.encode(), C.byref(v)))
    return v.value


def sample_source_rows(n, n_s=8192):
    """Diagnostics: gallery rows the bootstrap sample image of an n-row shard is drawn from."""
    import numpy as np
    f = load().mi_debug_sample_source_row
    return np.array([f(i, n, n_s) for i in range(n_s)], dtype=np.int64)


def device_count():
    n = C.c_int()
    check(load().mi_device_count(C.byref(n)))
    return n.value


class OnlineChain(_Handle):
    """mi_online_*: search -> qge1 expansion -> re-search (src/online.py:108-152) behind one coalescing worker thread of the
    LIBRARY.  `query` blocks inside the C call -- ctypes releases the interpreter lock -- so the request threads of a Python
    server cost the interpreter one foreign call each.  g_rows None: the plain search.  The galleries must outlive it."""
    _DESTROY = "mi_online_destroy"

    def __init__(self, g_search, g_rows, k, k_qe=3, w=4.0, eps=1e-6, max_batch=128, max_wait_us=500):
        h = C.c_void_p()
        check(load().mi_online_create(g_search._h, None if g_rows is None else g_rows._h, k, k_qe, w, eps, max_batch,
                                      max_wait_us, C.byref(h)))
        super().__init__(h.value)                # (query() takes no lock: the library coalesces its callers)
        self.k, self.d = int(k), g_search.d
        self._keep = (g_search, g_rows)
        self._query = load().mi_online_query

    def query(self, ptr, nq, memspace, pending=False, producer_stream=None, scores=False):
        """ptr: [nq, d] float32 rows (host or device address); pending: device rows still being produced on producer_stream
        (None = the null stream).  -> idx int64 [nq, k] (, score float32 [nq, k]), host arrays."""
        if self._keep[0]._h is None or (self._keep[1] is not None and self._keep[1]._h is None):
            raise RuntimeError("the galleries of this online chain have been closed")
        idx = np.empty((nq, self.k), dtype=np.int64)
        sc = np.empty((nq, self.k), dtype=np.float32) if scores else None
        rc = self._query(self._h, ptr, nq, memspace, 1 if pending else 0, producer_stream,
                         idx.__array_interface__["data"][0], None if sc is None else sc.__array_interface__["data"][0])
        if rc:
            check(rc)
        return (idx, sc) if scores else idx

    def native_clients(self, desc_ptr, n_desc, threads, per_thread):
        """Diagnostics: `threads` request threads of the library in a closed loop (mi_debug_online_clients).
        -> (seconds, last answer of every thread int64 [threads, k])."""
        last = np.empty((threads, self.k), dtype=np.int64)
        sec = C.c_double()
        check(load().mi_debug_online_clients(self._h, desc_ptr, n_desc, threads, per_thread, last.ctypes.data, C.byref(sec)))
        return sec.value, last

    def stats(self):
        a, b = C.c_int64(), C.c_int64()
        check(load().mi_online_stats(self._h, C.byref(a), C.byref(b)))
        return {"chains": a.value, "requests": b.value}
