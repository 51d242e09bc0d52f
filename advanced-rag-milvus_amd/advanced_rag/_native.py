"""ctypes binding of libhbmrag.so (C ABI: include/hbmrag.h).

The library is the product's compute path; there is no Python or CPU fallback.
If the shared object is missing or no HIP device is present, loading or
`ShardHandle(...)` raises — callers fail loudly instead of degrading.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

from .staging import csr_of_queries

HR_F32, HR_F16 = 0, 1
HR_METRIC_IP, HR_METRIC_COSINE, HR_METRIC_L2 = 0, 1, 2
HR_METHOD_SEMANTIC, HR_METHOD_SPARSE, HR_METHOD_DOMAIN = 1, 2, 4
HR_MAX_TOPK = 256
# normalisation of one list's scores in the weighted score fusion (hr_fuse_scores_dev; the table is in include/hbmrag.h)
HR_NORM_COSINE, HR_NORM_ATAN, HR_NORM_ATAN_DIST, HR_NORM_MINMAX, HR_NORM_MINMAX_DIST = 0, 1, 2, 3, 4
# multi-list fusion (hr_fuse_lists_dev): the list limit and the two modes
HR_MAX_FUSE_LISTS = 16
HR_FUSE_RRF, HR_FUSE_WEIGHTED = 0, 1
# decay ranker (hr_decay_rerank_dev): curve codes, the identity normalisation (also hr_mmr_select_vec_dev's) and the float64
# column kind, valid only there
HR_DECAY_GAUSS, HR_DECAY_EXP, HR_DECAY_LINEAR = 0, 1, 2
HR_NORM_NONE = -1
# boost ranker (hr_boost_rerank_dev): functions per query, hr_boost_func::flags, and the codes of both modes
HR_MAX_BOOST_FUNCS = 8
HR_BOOST_ACTIVE, HR_BOOST_RANDOM = 1, 2
HR_BOOST_MULTIPLY, HR_BOOST_SUM = 0, 1
# late-interaction rerank (hr_maxsim_rerank_dev): query tokens per query and the token dimension
HR_MAX_QUERY_TOKENS = 64
HR_MAX_TOKEN_DIM = 256
HR_COL_F64 = 5        # beside HR_COL_I64 / HR_COL_F32 below
HR_MAX_DEEP_K = 16384   # hr_search_*_deep, hr_deep_topk_dev: offset + k
HR_N_PHASES = 10
PHASE_NAMES = ("prep", "dense_scan", "group_select", "refine", "topk",
               "sparse_scan", "sparse_select", "sparse_refine", "sparse_topk", "finish_fused")
HR_DEBUG_FINISH_MODE, HR_DEBUG_FAIL_NEXT_BUILD, HR_DEBUG_DENSE_KERNELS, HR_DEBUG_SPARSE_RPB, HR_DEBUG_GROUP_ROWS = 1, 2, 3, 4, 5
HR_DEBUG_NO_TRIM = 6
HR_DEBUG_NO_RANGE_CLAMP = 7
HR_DEBUG_MAXSIM_SCAN_BLOCKS = 8

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libhbmrag.so")

_lib = None
_lib_lock = threading.Lock()


class HbmRagError(RuntimeError):
    """HIP/runtime failure reported by libhbmrag (status 2..5)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libhbmrag status {status}: {message}")
        self.status = status


_c = ctypes
_SIGNATURES = {
    "hr_version": (_c.c_int, []),
    "hr_create": (_c.c_int, [_c.c_int, _c.c_int64, _c.c_int, _c.c_int, _c.c_int64, _c.POINTER(_c.c_void_p)]),
    "hr_destroy": (None, [_c.c_void_p]),
    "hr_last_error": (_c.c_char_p, [_c.c_void_p]),
    "hr_set_row_offset": (_c.c_int, [_c.c_void_p, _c.c_int64]),
    "hr_reserve": (_c.c_int, [_c.c_void_p, _c.c_int64]),
    "hr_add_dense": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64]),
    "hr_add_dense_raw": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64]),
    "hr_add_dense_raw_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "hr_add_sparse": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64]),
    "hr_finalize": (_c.c_int, [_c.c_void_p]),
    "hr_compact": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    "hr_save": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "hr_load": (_c.c_int, [_c.c_char_p, _c.c_int, _c.POINTER(_c.c_void_p)]),
    "hr_get_info": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int32), _c.POINTER(_c.c_int32),
                               _c.POINTER(_c.c_int64)]),
    "hr_num_rows": (_c.c_int64, [_c.c_void_p]),
    "hr_num_sparse_rows": (_c.c_int64, [_c.c_void_p]),
    "hr_device_bytes": (_c.c_int64, [_c.c_void_p]),
    "hr_dense_scan_bytes": (_c.c_int64, [_c.c_void_p]),
    "hr_search_dense": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                   _c.c_void_p]),
    "hr_search_dense_range": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_search_sparse": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                    _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_search_dense_dmask": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p]),
    "hr_search_sparse_dmask": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                          _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_filter_eval_expr_dev": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_filter_eval_dev": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                      _c.c_void_p, _c.c_void_p]),
    "hr_bm25_encode_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_int,
                                      _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_hash_tokenize_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p]),
    "hr_fuse_rrf": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int,
                               _c.c_double, _c.c_double, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p,
                               _c.c_void_p, _c.c_void_p]),
    "hr_fuse_scores": (_c.c_int, [_c.c_void_p] + [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int] * 3 +
                       [_c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_fuse_scores_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int] * 3 +
                           [_c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_void_p, _c.c_int, _c.c_void_p,
                            _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_fuse_lists_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                     _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                     _c.c_void_p]),
    "hr_search_dense_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_search_dense_range_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                             _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_search_sparse_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int64,
                                        _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p]),
    "hr_search_hybrid_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p]),
    "hr_hybrid_prep_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                      _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "hr_hybrid_scan_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                      _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "hr_hybrid_finish_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p]),
    "hr_fuse_rrf_dev": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                   _c.c_double, _c.c_double, _c.c_double, _c.c_int, _c.c_int, _c.c_void_p,
                                   _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_merge_topk_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                     _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_merge_topk_asc_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                     _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_post_lists_dev": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    "hr_stream_create": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_void_p)]),
    "hr_stream_destroy": (_c.c_int, [_c.c_int, _c.c_void_p]),
    "hr_set_scan_cus": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "hr_debug_option": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int]),
    "hr_rerank_linear_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_int, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_mmr_select_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                     _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_mmr_vec_scratch_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "hr_mmr_select_vec_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                         _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_group_select_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_boost_rerank_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                       _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_decay_rerank_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                       _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p]),
    "hr_maxsim_rerank_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                        _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_maxsim_scan_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                      _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_mask_drop_groups_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "hr_group_select_n_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int,
                                         _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_mask_keep_groups_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "hr_add_layernorm_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                            _c.c_int, _c.c_float, _c.c_void_p]),
    "hr_embed_layernorm_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_float, _c.c_int64,
                                              _c.c_int64, _c.c_void_p]),
    "hr_attention_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_float, _c.c_void_p]),
    "hr_attention_rows_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int64,
                                             _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_float,
                                             _c.c_void_p]),
    "hr_linear_rows_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int,
                                          _c.c_int64, _c.c_void_p]),
    "hr_attention_fr_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_float, _c.c_void_p]),
    "hr_encoder_tail_f16_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                           _c.c_int64, _c.c_int, _c.c_int, _c.c_float, _c.c_int, _c.c_void_p]),
    "hr_mask_rows_scratch_bytes": (_c.c_size_t, [_c.c_int64]),
    "hr_mask_rows_dev": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p]),
    "hr_get_dense_rows_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                         _c.c_void_p]),
    "hr_get_dense_rows": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "hr_get_sparse_rows_scratch_bytes": (_c.c_size_t, [_c.c_int64]),
    "hr_get_sparse_rows_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                          _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_get_sparse_rows": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64,
                                      _c.c_void_p]),
    "hr_search_dense_deep": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                        _c.c_void_p]),
    "hr_search_sparse_deep": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_float, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hr_deep_topk_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int]),
    "hr_deep_topk_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64,
                                    _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_search_dense_deep_after": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hr_search_sparse_deep_after": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p,
                                               _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_void_p, _c.c_int, _c.c_void_p,
                                               _c.c_void_p]),
    "hr_deep_topk_window_dev": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int64,
                                           _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hr_set_profiling": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "hr_last_kernel_ms": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    "hr_last_compact_ms": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libhbmrag.so (building nothing: run __graft_entry__.build() or `make` first)."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or os.environ.get("HBMRAG_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise FileNotFoundError(
                f"{p} not found: build it with `make -C advanced-rag-milvus_amd` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        try:
            # torch ships its own libamdhip64 with the same soname; import it first
            # so both sides share ONE HIP runtime (device pointers interoperate).
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the library itself
            pass
        L = ctypes.CDLL(p)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if path is None:
            _lib = L
        return L


def _vp(a) -> Optional[ctypes.c_void_p]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(int(a))  # raw device pointer (e.g. tensor.data_ptr())


class ShardHandle:
    """One GPU's shard: dense tiles + sparse postings, owned by libhbmrag."""

    def __init__(self, dim: int, dtype: int = HR_F16, metric: int = HR_METRIC_COSINE, sparse_dim: int = 0,
                 device: int = 0, _adopt: Optional[int] = None):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        if _adopt is not None:  # handle created by hr_load
            self._h = ctypes.c_void_p(_adopt)
            self.dim, self.dtype, self.metric, self.sparse_dim, self.device = dim, dtype, metric, sparse_dim, device
            return
        self.dim, self.dtype, self.metric, self.sparse_dim, self.device = dim, dtype, metric, sparse_dim, device
        rc = self._lib.hr_create(device, dim, dtype, metric, sparse_dim, ctypes.byref(self._h))
        if rc != 0:
            msg = (self._lib.hr_last_error(None) or b"").decode()
            self._h = ctypes.c_void_p()
            self._raise(rc, msg)

    # -- error mapping: HR_EINVAL -> ValueError (as the reference raises for bad
    #    collections/shapes, indexing.py:466-467); everything else -> HbmRagError
    def _raise(self, rc: int, msg: Optional[str] = None):
        if msg is None:
            msg = (self._lib.hr_last_error(self._h) or b"").decode()
        if rc == 1:
            raise ValueError(msg)
        raise HbmRagError(rc, msg)

    def _check(self, rc: int):
        if rc != 0:
            self._raise(rc)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.hr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- snapshot
    def save(self, path: str):
        self._check(self._lib.hr_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path: str, dim: int, dtype: int = HR_F16, metric: int = HR_METRIC_COSINE, sparse_dim: int = 0,
             device: int = 0) -> "ShardHandle":
        """Load a snapshot; dim/dtype/metric/sparse_dim describe what the caller expects and are checked against what
        the file holds (a mismatch would make later calls read query or row buffers of the wrong size)."""
        lib = load_library()
        h = ctypes.c_void_p()
        rc = lib.hr_load(os.fsencode(path), device, ctypes.byref(h))
        if rc != 0:
            msg = (lib.hr_last_error(None) or b"").decode()
            if rc == 1:
                raise ValueError(msg)
            raise HbmRagError(rc, msg)
        f_dim, f_sdim = ctypes.c_int64(), ctypes.c_int64()
        f_dtype, f_metric = ctypes.c_int32(), ctypes.c_int32()
        lib.hr_get_info(h, ctypes.byref(f_dim), ctypes.byref(f_dtype), ctypes.byref(f_metric), ctypes.byref(f_sdim))
        got = (f_dim.value, f_dtype.value, f_metric.value, f_sdim.value)
        if got != (dim, dtype, metric, sparse_dim):
            lib.hr_destroy(h)
            raise ValueError(f"snapshot {path} holds (dim, dtype, metric, sparse_dim) = {got}, expected "
                             f"{(dim, dtype, metric, sparse_dim)}")
        return cls(dim, dtype, metric, sparse_dim, device, _adopt=h.value)

    # -- ingest
    row_offset = 0    # global id of local row 0 as set through this object (a loaded snapshot carries its own)

    def set_row_offset(self, first_row: int):
        self._check(self._lib.hr_set_row_offset(self._h, first_row))
        self.row_offset = int(first_row)

    def reserve(self, n_rows: int):
        self._check(self._lib.hr_reserve(self._h, n_rows))

    def add_dense(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n,{self.dim}], got {rows.shape}")
        if rows.dtype == np.float32 and self.dtype == HR_F16:
            self._check(self._lib.hr_add_dense(self._h, _vp(rows), rows.shape[0]))
        elif (rows.dtype == np.float16 and self.dtype == HR_F16) or (rows.dtype == np.float32 and self.dtype == HR_F32):
            self._check(self._lib.hr_add_dense_raw(self._h, _vp(rows), rows.shape[0]))
        else:
            raise ValueError(f"cannot ingest {rows.dtype} rows into this shard")

    def add_dense_dev(self, d_ptr: int, n: int, stream: int = 0):
        self._check(self._lib.hr_add_dense_raw_dev(self._h, _vp(d_ptr), n, _vp(stream) if stream else None))

    def add_sparse(self, indptr: np.ndarray, indices: np.ndarray, values: np.ndarray):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float32)
        self._check(self._lib.hr_add_sparse(self._h, _vp(indptr), _vp(indices), _vp(values), indptr.shape[0] - 1))

    def finalize(self):
        self._check(self._lib.hr_finalize(self._h))

    def compact(self, keep=None, d_keep: int = 0) -> Tuple[int, int]:
        """hr_compact: remove the rows whose keep bit is 0 for good; returns (dense rows, sparse rows) left.
        keep = boolean array (one entry per local row) or packed uint8 mask (bit r % 8 of byte r // 8), or d_keep =
        device pointer of a packed mask of 8 * ceil(n / 64) bytes, n = max(num_rows, num_sparse_rows).  The handle must
        be finalized; no search may run meanwhile, and row numbers and row masks held by the caller are void afterwards."""
        kd, ks = ctypes.c_int64(0), ctypes.c_int64(0)
        if d_keep:
            self._check(self._lib.hr_compact(self._h, _vp(d_keep), 1, ctypes.byref(kd), ctypes.byref(ks)))
            return kd.value, ks.value
        if keep is None:
            raise ValueError("compact needs a keep mask")
        n = max(self.num_rows, self.num_sparse_rows)
        m = np.asarray(keep)
        if m.dtype == np.bool_:
            if m.ndim != 1 or m.shape[0] != n:
                raise ValueError(f"boolean keep mask has shape {m.shape}, the shard holds {n} rows")
            m = np.packbits(m, bitorder="little")
        m = self._mask(m, n)
        self._check(self._lib.hr_compact(self._h, _vp(m), 0, ctypes.byref(kd), ctypes.byref(ks)))
        return kd.value, ks.value

    @property
    def num_rows(self) -> int:
        return int(self._lib.hr_num_rows(self._h))

    @property
    def num_sparse_rows(self) -> int:
        return int(self._lib.hr_num_sparse_rows(self._h))

    @property
    def device_bytes(self) -> int:
        return int(self._lib.hr_device_bytes(self._h))

    @property
    def dense_scan_bytes(self) -> int:
        return int(self._lib.hr_dense_scan_bytes(self._h))

    # -- read path
    def get_dense_rows(self, rows) -> np.ndarray:
        """hr_get_dense_rows: the stored vectors of the rows with the given GLOBAL ids (local row + row offset; any
        order, repeats allowed) as float32 [n, dim], fp16 shards widened exactly.  An id outside the shard: ValueError."""
        ids = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = np.empty((ids.shape[0], self.dim), dtype=np.float32)
        self._check(self._lib.hr_get_dense_rows(self._h, _vp(ids), ids.shape[0], _vp(out)))
        return out

    def get_dense_rows_dev(self, d_rows: int, n: int, out_dtype: int, d_out: int, out_stride: int = 0, d_missing: int = 0,
                           stream: int = 0):
        """hr_get_dense_rows_dev (device pointers, asynchronous on `stream`): row i of d_out = the stored row d_rows[i] as
        out_dtype (HR_F32, or HR_F16 on an fp16 shard); out_stride in elements (0 = dim); an id outside the shard gives a
        row of zeros and is counted in the int32 at d_missing (0 = not wanted)."""
        self._check(self._lib.hr_get_dense_rows_dev(self._h, _vp(d_rows) if d_rows else None, n, out_dtype,
                                                    _vp(d_out) if d_out else None, out_stride or self.dim,
                                                    _vp(d_missing) if d_missing else None, _vp(stream) if stream else None))

    def mmr_vec_scratch_bytes(self, B: int, k_in: int) -> int:
        """hr_mmr_vec_scratch_bytes: the bytes of d_scratch that mmr_select_vec_dev needs for B lists of k_in entries."""
        return int(self._lib.hr_mmr_vec_scratch_bytes(self._h, B, k_in))

    def mmr_select_vec_dev(self, d_ids: int, d_scores: int, score_is_f64: bool, norm: int, d_n: int, B: int, k_in: int,
                           d_lambda: int, k_out: int, d_scratch: int, d_out_pos: int, d_out_val: int, d_out_n: int,
                           stream: int = 0):
        """hr_mmr_select_vec_dev (device pointers; 0 = NULL; asynchronous on `stream`): greedy MMR over B ranked lists on
        the cosine of the stored rows, lambda per query at d_lambda -> list positions in pick order, the value of every
        pick, the picks per query."""
        p = lambda x: _vp(x) if x else None  # noqa: E731
        self._check(self._lib.hr_mmr_select_vec_dev(self._h, p(d_ids), p(d_scores), 1 if score_is_f64 else 0, norm, p(d_n), B, k_in,
                                                    p(d_lambda), k_out, p(d_scratch), p(d_out_pos), p(d_out_val), p(d_out_n),
                                                    p(stream)))

    def get_sparse_rows(self, rows) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """hr_get_sparse_rows: the stored sparse rows with the given GLOBAL ids (any order, repeats allowed) as one CSR
        (indptr int64 [n + 1], indices int32 [nnz], values float32 [nnz]): the sizing call, then the fetch.  An id outside
        the shard: ValueError."""
        ids = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = ids.shape[0]
        indptr = np.zeros(n + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        self._check(self._lib.hr_get_sparse_rows(self._h, _vp(ids), n, _vp(indptr), None, None, 0, ctypes.byref(total)))
        nnz = int(total.value)
        indices, values = np.empty(nnz, dtype=np.int32), np.empty(nnz, dtype=np.float32)
        if nnz:
            self._check(self._lib.hr_get_sparse_rows(self._h, _vp(ids), n, _vp(indptr), _vp(indices), _vp(values), nnz,
                                                     ctypes.byref(total)))
            if int(total.value) != nnz:  # an append or a compaction between the two calls
                raise HbmRagError(2, "the sparse rows changed between the sizing call and the fetch")
        return indptr, indices, values

    def get_sparse_rows_dev(self, d_rows: int, n: int, d_out_indptr: int, d_out_idx: int, d_out_val: int, cap: int, d_counts: int,
                            d_scratch: int, stream: int = 0):
        """hr_get_sparse_rows_dev (device pointers, asynchronous on `stream`): the stored rows d_rows[0 .. n) as a CSR in
        d_out_indptr [n + 1] / d_out_idx / d_out_val (capacity `cap` entries; 0 with null entry buffers = sizes only);
        d_counts[0] = all entries, d_counts[1] = ids outside the shard (empty rows); d_scratch =
        get_sparse_rows_scratch_bytes(n) bytes."""
        p = lambda x: _vp(x) if x else None  # noqa: E731
        self._check(self._lib.hr_get_sparse_rows_dev(self._h, p(d_rows), n, p(d_out_indptr), p(d_out_idx), p(d_out_val), cap,
                                                     p(d_counts), p(d_scratch), p(stream)))

    # -- search, host buffers
    @staticmethod
    def _mask(rowmask, n_rows: int):
        """The library copies (n_rows + 7) // 8 bytes of a row mask: a shorter buffer would be over-read."""
        if rowmask is None:
            return None
        m = np.ascontiguousarray(rowmask, dtype=np.uint8)
        if m.size < (n_rows + 7) // 8:
            raise ValueError(f"row mask has {m.size} bytes, the collection's {n_rows} rows need {(n_rows + 7) // 8}")
        return m

    def search_dense(self, q: np.ndarray, k: int, rowmask: Optional[np.ndarray] = None,
                     d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """rowmask = packed host mask (uploaded), or d_rowmask = device pointer of a mask already in HBM."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32)
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != shard dim {self.dim}")
        B = q.shape[0]
        ids = np.empty((B, k), dtype=np.int64)
        sc = np.empty((B, k), dtype=np.float32)
        if d_rowmask:
            self._check(self._lib.hr_search_dense_dmask(self._h, _vp(q), B, k, _vp(d_rowmask), _vp(ids), _vp(sc)))
            return ids, sc
        m = self._mask(rowmask, self.num_rows)
        self._check(self._lib.hr_search_dense(self._h, _vp(q), B, k, _vp(m), _vp(ids), _vp(sc)))
        return ids, sc

    @staticmethod
    def _bounds(b, B: int, name: str):
        """One side of a range search's bounds: None (unbounded), a number for every query, or B numbers."""
        if b is None:
            return None
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float64), (B,)))
        if np.isnan(a).any():
            raise ValueError(f"{name} of query {int(np.flatnonzero(np.isnan(a))[0])} is NaN")
        return a

    def search_dense_range(self, q: np.ndarray, k: int, radius=None, range_filter=None,
                           rowmask: Optional[np.ndarray] = None, d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Range search (hr_search_dense_range): the best k rows among those whose canonical score lies in the range
        (COSINE, IP: radius < score <= range_filter; L2: range_filter <= distance < radius).  radius / range_filter:
        None = unbounded, one number, or one per query.  An empty interval raises ValueError (HR_EINVAL)."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32)
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != shard dim {self.dim}")
        B = q.shape[0]
        r, f = self._bounds(radius, B, "radius"), self._bounds(range_filter, B, "range_filter")
        ids = np.empty((B, k), dtype=np.int64)
        sc = np.empty((B, k), dtype=np.float32)
        m = d_rowmask if d_rowmask else self._mask(rowmask, self.num_rows)
        self._check(self._lib.hr_search_dense_range(self._h, _vp(q), B, k, _vp(m),
                                                    1 if d_rowmask else 0, _vp(r), _vp(f), _vp(ids), _vp(sc)))
        return ids, sc

    def search_sparse(self, queries: Sequence[Tuple[Sequence[int], Sequence[float]]], k: int,
                      drop_ratio: float = 0.0, rowmask: Optional[np.ndarray] = None,
                      d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        B = len(queries)
        indptr, idx, val = csr_of_queries(queries)
        ids = np.empty((B, k), dtype=np.int64)
        sc = np.empty((B, k), dtype=np.float32)
        if d_rowmask:
            self._check(self._lib.hr_search_sparse_dmask(self._h, _vp(indptr), _vp(idx), _vp(val), B, k, float(drop_ratio),
                                                         _vp(d_rowmask), _vp(ids), _vp(sc)))
            return ids, sc
        m = self._mask(rowmask, self.num_sparse_rows)
        self._check(self._lib.hr_search_sparse(self._h, _vp(indptr), _vp(idx), _vp(val), B, k, float(drop_ratio),
                                               _vp(m), _vp(ids), _vp(sc)))
        return ids, sc

    def search_dense_deep(self, q: np.ndarray, k: int, offset: int = 0, rowmask: Optional[np.ndarray] = None,
                          d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Deep search (hr_search_dense_deep): entries offset .. offset + k - 1 of the collection's exact ranking,
        offset + k <= HR_MAX_DEEP_K.  Every row is refined: a call reads the whole shard once per query."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32)
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != shard dim {self.dim}")
        B = q.shape[0]
        ids = np.empty((B, max(k, 0)), dtype=np.int64)
        sc = np.empty((B, max(k, 0)), dtype=np.float32)
        m = d_rowmask if d_rowmask else self._mask(rowmask, self.num_rows)
        self._check(self._lib.hr_search_dense_deep(self._h, _vp(q), B, k, offset, _vp(m), 1 if d_rowmask else 0, _vp(ids),
                                                   _vp(sc)))
        return ids, sc

    def search_sparse_deep(self, queries: Sequence[Tuple[Sequence[int], Sequence[float]]], k: int, offset: int = 0,
                           drop_ratio: float = 0.0, rowmask: Optional[np.ndarray] = None,
                           d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Deep search of the sparse collection (hr_search_sparse_deep); only rows with a positive score are ranked."""
        B = len(queries)
        indptr, idx, val = csr_of_queries(queries)
        ids = np.empty((B, max(k, 0)), dtype=np.int64)
        sc = np.empty((B, max(k, 0)), dtype=np.float32)
        m = d_rowmask if d_rowmask else self._mask(rowmask, self.num_sparse_rows)
        self._check(self._lib.hr_search_sparse_deep(self._h, _vp(indptr), _vp(idx), _vp(val), B, k, offset, float(drop_ratio),
                                                    _vp(m), 1 if d_rowmask else 0, _vp(ids), _vp(sc)))
        return ids, sc

    @staticmethod
    def _cursor(after, B: int):
        """The cursor operand of the *_deep_after forms: None, or (scores [B], ids [B]) / (scores, ids, has [B]) -> the three
        arrays the library reads (all None = no query has a cursor)."""
        if after is None:
            return None, None, None
        score = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float32), (B,)))
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64), (B,)))
        has = np.ones(B, np.uint8) if len(after) < 3 or after[2] is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(after[2]), (B,)).astype(bool), dtype=np.uint8)
        return score, ids, has

    def search_dense_deep_after(self, q: np.ndarray, k: int, after=None, bounds=None, rowmask: Optional[np.ndarray] = None,
                                d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The search iterator's page (hr_search_dense_deep_after): the first k <= HR_MAX_DEEP_K entries of the collection's
        exact ranking that come strictly after the cursor `after` = (scores [B], ids [B][, has [B]]), None = from the top.
        bounds = (radius, range_filter) of a range search, each None, a number or one per query: float64 as in
        search_dense_range, handed to the library as the fp32 that keeps the same fp32 scores (f32_bound)."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32)
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != shard dim {self.dim}")
        B = q.shape[0]
        a_sc, a_id, a_has = self._cursor(after, B)
        up = self.metric == HR_METRIC_L2
        r, f = (None, None) if bounds is None else (self._bounds(bounds[0], B, "radius"), self._bounds(bounds[1], B, "range_filter"))
        r, f = (None if r is None else f32_bound(r, up)), (None if f is None else f32_bound(f, up))
        ids = np.empty((B, max(k, 0)), dtype=np.int64)
        sc = np.empty((B, max(k, 0)), dtype=np.float32)
        m = d_rowmask if d_rowmask else self._mask(rowmask, self.num_rows)
        self._check(self._lib.hr_search_dense_deep_after(self._h, _vp(q), B, k, _vp(a_sc), _vp(a_id), _vp(a_has), _vp(r), _vp(f),
                                                         _vp(m), 1 if d_rowmask else 0, _vp(ids), _vp(sc)))
        return ids, sc

    def search_sparse_deep_after(self, queries: Sequence[Tuple[Sequence[int], Sequence[float]]], k: int, after=None,
                                 drop_ratio: float = 0.0, rowmask: Optional[np.ndarray] = None,
                                 d_rowmask: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """hr_search_sparse_deep_after: the sparse ranking (positive scores only) after the cursor, as search_dense_deep_after."""
        B = len(queries)
        indptr, idx, val = csr_of_queries(queries)
        a_sc, a_id, a_has = self._cursor(after, B)
        ids = np.empty((B, max(k, 0)), dtype=np.int64)
        sc = np.empty((B, max(k, 0)), dtype=np.float32)
        m = d_rowmask if d_rowmask else self._mask(rowmask, self.num_sparse_rows)
        self._check(self._lib.hr_search_sparse_deep_after(self._h, _vp(indptr), _vp(idx), _vp(val), B, k, _vp(a_sc), _vp(a_id),
                                                          _vp(a_has), float(drop_ratio), _vp(m), 1 if d_rowmask else 0, _vp(ids),
                                                          _vp(sc)))
        return ids, sc

    def fuse_rrf(self, ids_a, ids_b, ids_c=(), wa: float = 0.7, wb: float = 0.3, wc: float = 0.2, rrf_k: int = 60):
        a = np.ascontiguousarray(ids_a, dtype=np.int64)
        b = np.ascontiguousarray(ids_b, dtype=np.int64)
        c = np.ascontiguousarray(ids_c, dtype=np.int64)
        cap = max(len(a) + len(b) + len(c), 1)
        oi = np.empty(cap, dtype=np.int64)
        os_ = np.empty(cap, dtype=np.float64)
        om = np.empty(cap, dtype=np.int32)
        n = ctypes.c_int32(0)
        self._check(self._lib.hr_fuse_rrf(self._h, _vp(a) if len(a) else None, len(a), _vp(b) if len(b) else None,
                                          len(b), _vp(c) if len(c) else None, len(c), wa, wb, wc, rrf_k, _vp(oi),
                                          _vp(os_), _vp(om), ctypes.byref(n)))
        return oi[:n.value].copy(), os_[:n.value].copy(), om[:n.value].copy()

    def fuse_scores(self, lists, norms, weights=(0.7, 0.3, 0.2)):
        """hr_fuse_scores: weighted score fusion of up to three (ids, fp32 scores) lists of one query; norms = one
        HR_NORM_* code per list.  -> (ids, float64 fused scores, method bit masks) in fused order."""
        lists = list(lists) + [((), ())] * (3 - len(lists))
        norms = list(norms) + [HR_NORM_COSINE] * (3 - len(norms))
        w = list(weights) + [0.0] * (3 - len(weights))
        ids = [np.ascontiguousarray(l[0], dtype=np.int64) for l in lists]
        sc = [np.ascontiguousarray(l[1], dtype=np.float32) for l in lists]
        if any(len(i) != len(s) for i, s in zip(ids, sc)):
            raise ValueError("a list's ids and scores differ in length")
        cap = max(sum(len(i) for i in ids), 1)
        oi = np.empty(cap, dtype=np.int64)
        os_ = np.empty(cap, dtype=np.float64)
        om = np.empty(cap, dtype=np.int32)
        n = ctypes.c_int32(0)
        args = []
        for i, s, code in zip(ids, sc, norms):
            args += [_vp(i) if len(i) else None, _vp(s) if len(i) else None, len(i), int(code)]
        self._check(self._lib.hr_fuse_scores(self._h, *args, float(w[0]), float(w[1]), float(w[2]), _vp(oi), _vp(os_),
                                             _vp(om), ctypes.byref(n)))
        return oi[:n.value].copy(), os_[:n.value].copy(), om[:n.value].copy()

    # -- search, device buffers (raw pointers; asynchronous on `stream`)
    def search_dense_dev(self, d_q: int, B: int, k: int, d_ids: int, d_scores: int, d_flags: int = 0,
                         d_rowmask: int = 0, stream: int = 0):
        self._check(self._lib.hr_search_dense_dev(self._h, _vp(d_q), B, k, _vp(d_rowmask) if d_rowmask else None,
                                                  _vp(d_ids), _vp(d_scores), _vp(d_flags) if d_flags else None,
                                                  _vp(stream) if stream else None))

    def search_dense_range_dev(self, d_q: int, B: int, k: int, d_radius: int, d_range_filter: int, d_ids: int,
                               d_scores: int, d_flags: int = 0, d_rowmask: int = 0, stream: int = 0):
        """d_radius / d_range_filter: device pointers of B float64 each, 0 = that side unbounded for every query."""
        self._check(self._lib.hr_search_dense_range_dev(
            self._h, _vp(d_q), B, k, _vp(d_rowmask) if d_rowmask else None, _vp(d_radius) if d_radius else None,
            _vp(d_range_filter) if d_range_filter else None, _vp(d_ids), _vp(d_scores),
            _vp(d_flags) if d_flags else None, _vp(stream) if stream else None))

    def search_sparse_dev(self, d_indptr: int, d_idx: int, d_val: int, B: int, nnz_total: int, max_q_nnz: int, k: int,
                          d_ids: int, d_scores: int, d_flags: int = 0, d_rowmask: int = 0, stream: int = 0):
        self._check(self._lib.hr_search_sparse_dev(self._h, _vp(d_indptr), _vp(d_idx), _vp(d_val), B, nnz_total,
                                                   max_q_nnz, k, _vp(d_rowmask) if d_rowmask else None, _vp(d_ids),
                                                   _vp(d_scores), _vp(d_flags) if d_flags else None,
                                                   _vp(stream) if stream else None))

    def search_hybrid_dev(self, d_q: int, d_indptr: int, d_idx: int, d_val: int, B: int, nnz_total: int,
                          max_q_nnz: int, k: int, d_ids: int, d_scores: int, d_flags: int = 0, d_rowmask: int = 0,
                          stream: int = 0):
        """Dense + sparse lists of one batch in one call ([2][B][k] outputs; dense first)."""
        self._check(self._lib.hr_search_hybrid_dev(self._h, _vp(d_q), _vp(d_indptr), _vp(d_idx) if d_idx else None,
                                                   _vp(d_val) if d_val else None, B, nnz_total, max_q_nnz, k,
                                                   _vp(d_rowmask) if d_rowmask else None, _vp(d_ids), _vp(d_scores),
                                                   _vp(d_flags) if d_flags else None, _vp(stream) if stream else None))

    def hybrid_prep_dev(self, d_q: int, d_indptr: int, d_idx: int, d_val: int, B: int, nnz_total: int, max_q_nnz: int,
                        k: int, slot: int, stream: int = 0):
        """Query preparation of `slot` alone, on `stream`; the next hybrid_scan_dev on the slot enqueues the scans only."""
        self._check(self._lib.hr_hybrid_prep_dev(self._h, _vp(d_q), _vp(d_indptr), _vp(d_idx) if d_idx else None,
                                                 _vp(d_val) if d_val else None, B, nnz_total, max_q_nnz, k, slot,
                                                 _vp(stream) if stream else None))

    def hybrid_scan_dev(self, d_q: int, d_indptr: int, d_idx: int, d_val: int, B: int, nnz_total: int, max_q_nnz: int,
                        k: int, slot: int, stream: int = 0, d_rowmask: int = 0):
        self._check(self._lib.hr_hybrid_scan_dev(self._h, _vp(d_q), _vp(d_indptr), _vp(d_idx) if d_idx else None,
                                                 _vp(d_val) if d_val else None, B, nnz_total, max_q_nnz, k,
                                                 _vp(d_rowmask) if d_rowmask else None, slot,
                                                 _vp(stream) if stream else None))

    def hybrid_finish_dev(self, d_q: int, d_indptr: int, d_idx: int, d_val: int, B: int, max_q_nnz: int, k: int,
                          slot: int, d_ids: int, d_scores: int, d_flags: int = 0, stream: int = 0, d_rowmask: int = 0):
        self._check(self._lib.hr_hybrid_finish_dev(self._h, _vp(d_q), _vp(d_indptr), _vp(d_idx) if d_idx else None,
                                                   _vp(d_val) if d_val else None, B, max_q_nnz, k,
                                                   _vp(d_rowmask) if d_rowmask else None, slot, _vp(d_ids),
                                                   _vp(d_scores), _vp(d_flags) if d_flags else None,
                                                   _vp(stream) if stream else None))

    def set_scan_cus(self, n_cus: int):
        """Compute units the scans' stream may occupy (0 = all): sizes their persistent grids (hr_stream_create masks)."""
        self._check(self._lib.hr_set_scan_cus(self._h, int(n_cus)))

    def debug_option(self, key: int, value: int):
        self._check(self._lib.hr_debug_option(self._h, key, value))

    # -- measurement
    def set_profiling(self, level: int):
        self._check(self._lib.hr_set_profiling(self._h, level))

    def kernel_ms(self):
        """{phase: (mean ms per launch, launches)} since the previous call."""
        buf = np.zeros(2 * HR_N_PHASES, dtype=np.float32)
        self._check(self._lib.hr_last_kernel_ms(self._h, _vp(buf), buf.shape[0]))
        return {PHASE_NAMES[p]: (float(buf[p]), int(buf[HR_N_PHASES + p])) for p in range(HR_N_PHASES)}

    def compact_ms(self):
        """The last compact() that changed the shard: ms of the tile gather (device events; 0 without set_profiling), of
        the whole call and of the posting rebuild inside it (host wall time)."""
        buf = np.zeros(3, dtype=np.float32)
        self._check(self._lib.hr_last_compact_ms(self._h, _vp(buf), 3))
        return {"tile_gather": float(buf[0]), "call": float(buf[1]), "posting_rebuild": float(buf[2])}


def fuse_rrf_dev(d_a: int, ka: int, d_b: int, kb: int, d_c: int, kc: int, B: int, wa: float, wb: float, wc: float,
                 rrf_k: int, top_k: int, d_out_ids: int, d_out_scores: int, d_out_methods: int, d_n_out: int,
                 stream: int = 0):
    L = load_library()
    rc = L.hr_fuse_rrf_dev(_vp(d_a) if ka else None, ka, _vp(d_b) if kb else None, kb, _vp(d_c) if kc else None, kc,
                           B, wa, wb, wc, rrf_k, top_k, _vp(d_out_ids), _vp(d_out_scores), _vp(d_out_methods),
                           _vp(d_n_out), _vp(stream) if stream else None)
    if rc != 0:
        msg = (L.hr_last_error(None) or b"").decode()
        if rc == 1:
            raise ValueError(msg)
        raise HbmRagError(rc, msg)


def _raise_global(L, rc: int):
    msg = (L.hr_last_error(None) or b"").decode()
    if rc == 1:
        raise ValueError(msg)
    raise HbmRagError(rc, msg)


def fuse_scores_dev(d_a: int, d_sa: int, ka: int, norm_a: int, d_b: int, d_sb: int, kb: int, norm_b: int, d_c: int,
                    d_sc: int, kc: int, norm_c: int, B: int, wa: float, wb: float, wc: float, d_w_query: int, top_k: int,
                    d_out_ids: int, d_out_scores: int, d_out_methods: int, d_n_out: int, stream: int = 0):
    """hr_fuse_scores_dev: weighted score fusion of a batch (device pointers; 0 = NULL; norm_* = HR_NORM_* per list)."""
    L = load_library()
    p = lambda v: _vp(v) if v else None
    rc = L.hr_fuse_scores_dev(p(d_a), p(d_sa), ka, norm_a, p(d_b), p(d_sb), kb, norm_b, p(d_c), p(d_sc), kc, norm_c, B,
                              wa, wb, wc, p(d_w_query), top_k, p(d_out_ids), p(d_out_scores), p(d_out_methods),
                              p(d_n_out), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def fuse_lists_dev(d_ids: int, d_scores: int, n_lists: int, k_in: int, B: int, mode: int, rrf_k: int, norms, weights,
                   d_w_query: int, top_k: int, d_out_ids: int, d_out_scores: int, d_out_lists: int, d_n_out: int,
                   stream: int = 0):
    """hr_fuse_lists_dev: fusion of n_lists ranked lists per query (device pointers; 0 = NULL).  norms: n_lists HR_NORM_*
    codes or None (host side), weights: n_lists numbers or None (host side; d_w_query then carries them per query)."""
    L = load_library()
    p = lambda v: _vp(v) if v else None
    h_norms = None if norms is None else np.ascontiguousarray(norms, dtype=np.int32)
    h_w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    for name, arr in (("norms", h_norms), ("weights", h_w)):
        if arr is not None and arr.shape != (max(int(n_lists), 0),):
            raise ValueError(f"{name} must hold one value per list ({n_lists}), got shape {arr.shape}")
    rc = L.hr_fuse_lists_dev(p(d_ids), p(d_scores), n_lists, k_in, B, mode, rrf_k, _vp(h_norms), _vp(h_w), p(d_w_query),
                             top_k, p(d_out_ids), p(d_out_scores), p(d_out_lists), p(d_n_out), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def mmr_select_dev(d_ids: int, d_scores: int, d_n: int, B: int, k_in: int, d_tok_indptr: int, d_tok: int, tok_rows: int,
                   first_row: int, d_lambda: int, k_out: int, d_out_pos: int, d_out_n: int, stream: int = 0):
    """hr_mmr_select_dev: greedy MMR over a batch of fused lists (device pointers; 0 = NULL)."""
    L = load_library()
    rc = L.hr_mmr_select_dev(_vp(d_ids) if d_ids else None, _vp(d_scores) if d_scores else None, _vp(d_n) if d_n else None,
                             B, k_in, _vp(d_tok_indptr) if d_tok_indptr else None, _vp(d_tok) if d_tok else None,
                             tok_rows, first_row, _vp(d_lambda) if d_lambda else None, k_out,
                             _vp(d_out_pos) if d_out_pos else None, _vp(d_out_n) if d_out_n else None,
                             _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def group_select_dev(d_ids: int, d_n: int, B: int, k_in: int, d_keys: int, key_rows: int, first_row: int, k_out: int,
                     d_out_pos: int, d_out_keys: int, d_out_n: int, d_flags: int, stream: int = 0):
    """hr_group_select_dev: the first entry of every group of a batch of ranked lists (device pointers; 0 = NULL)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_group_select_dev(p(d_ids), p(d_n), B, k_in, p(d_keys), key_rows, first_row, k_out, p(d_out_pos), p(d_out_keys),
                               p(d_out_n), p(d_flags), p(stream))
    if rc != 0:
        _raise_global(L, rc)


# one query's operands of hr_decay_rerank_dev (struct hr_decay_query): origin, offset, coef as float64, func and a reserved int32
DECAY_QUERY_DTYPE = np.dtype([("origin", "<f8"), ("offset", "<f8"), ("coef", "<f8"), ("func", "<i4"), ("reserved", "<i4")])


def decay_rerank_dev(d_ids: int, d_scores: int, score_is_f64: bool, d_n: int, B: int, k_in: int, d_col: int, col_kind: int,
                     col_rows: int, first_row: int, d_params: int, norm: int, k_out: int, d_out_pos: int, d_out_ids: int,
                     d_out_scores: int, d_out_n: int, stream: int = 0):
    """hr_decay_rerank_dev: the decay ranker over a batch of ranked lists (device pointers; 0 = NULL; d_params = [B]
    records of DECAY_QUERY_DTYPE on the device)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_decay_rerank_dev(p(d_ids), p(d_scores), 1 if score_is_f64 else 0, p(d_n), B, k_in, p(d_col), col_kind, col_rows,
                               first_row, p(d_params), norm, k_out, p(d_out_pos), p(d_out_ids), p(d_out_scores), p(d_out_n),
                               p(stream))
    if rc != 0:
        _raise_global(L, rc)


# one function of hr_boost_rerank_dev (struct hr_boost_func, 56 bytes): two device pointers, their row counts, weight, seed, flags
BOOST_FUNC_DTYPE = np.dtype([("mask", "<u8"), ("key_col", "<u8"), ("mask_rows", "<i8"), ("key_rows", "<i8"), ("weight", "<f8"),
                             ("seed", "<u8"), ("flags", "<i4"), ("reserved", "<i4")])


def boost_rerank_dev(d_ids: int, d_scores: int, score_is_f64: bool, d_n: int, B: int, k_in: int, d_funcs: int, n_funcs: int,
                     first_row: int, function_mode: int, boost_mode: int, norm: int, ascending: bool, k_out: int,
                     d_out_pos: int, d_out_ids: int, d_out_scores: int, d_out_matched: int, d_out_n: int, stream: int = 0):
    """hr_boost_rerank_dev: the boost ranker over a batch of ranked lists (device pointers; 0 = NULL; d_funcs = [B, n_funcs]
    records of BOOST_FUNC_DTYPE on the device)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_boost_rerank_dev(p(d_ids), p(d_scores), 1 if score_is_f64 else 0, p(d_n), B, k_in, p(d_funcs), n_funcs, first_row,
                               function_mode, boost_mode, norm, 1 if ascending else 0, k_out, p(d_out_pos), p(d_out_ids),
                               p(d_out_scores), p(d_out_matched), p(d_out_n), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def maxsim_rerank_dev(d_ids: int, d_n: int, B: int, k_in: int, d_qtok: int, d_qn: int, tq_stride: int, dim: int, d_indptr: int,
                      d_tok: int, tok_rows: int, first_row: int, k_out: int, d_out_pos: int, d_out_ids: int, d_out_scores: int,
                      d_out_n: int, stream: int = 0):
    """hr_maxsim_rerank_dev: the late-interaction rerank over a batch of ranked lists (device pointers; 0 = NULL; d_qtok =
    fp16 [B, tq_stride, dim], d_qn = int32 [B], the token store as CSR over rows first_row .. first_row + tok_rows)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_maxsim_rerank_dev(p(d_ids), p(d_n), B, k_in, p(d_qtok), p(d_qn), tq_stride, dim, p(d_indptr), p(d_tok), tok_rows,
                                first_row, k_out, p(d_out_pos), p(d_out_ids), p(d_out_scores), p(d_out_n), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def maxsim_scan_dev(d_qtok: int, d_qn: int, B: int, tq_stride: int, dim: int, d_indptr: int, d_tok: int, tok_rows: int, n_rows: int,
                    d_rowmask: int, d_scores: int, d_rows: int, stream: int = 0):
    """hr_maxsim_scan_dev: the MaxSim score of every local row for B queries (device pointers; 0 = NULL; d_qtok = fp16
    [B, tq_stride, dim], d_qn = int32 [B], d_rowmask packed or 0 = all rows) -> d_scores fp32 / d_rows int32 [B, n_rows],
    the candidate arrays deep_topk_dev selects from."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_maxsim_scan_dev(p(d_qtok), p(d_qn), B, tq_stride, dim, p(d_indptr), p(d_tok), tok_rows, n_rows, p(d_rowmask),
                              p(d_scores), p(d_rows), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def mask_rows_scratch_bytes(n_rows: int) -> int:
    """hr_mask_rows_scratch_bytes: device scratch hr_mask_rows_dev needs for a mask of n_rows rows."""
    return int(load_library().hr_mask_rows_scratch_bytes(n_rows))


def f32_bound(x, up: bool) -> np.ndarray:
    """A range bound given as float64 -> the fp32 that cuts the fp32 scores at the same place: the largest fp32 <= x (COSINE
    and IP: score > x and score <= x both hold for the same fp32 scores as with x rounded down), up=True the smallest fp32
    >= x (L2: distance >= x, distance < x)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = np.atleast_1d(x.astype(np.float32))
    x = np.atleast_1d(x)
    off = (f.astype(np.float64) < x) if up else (f.astype(np.float64) > x)
    f[off] = np.nextafter(f[off], np.float32(np.inf if up else -np.inf))
    return np.ascontiguousarray(f)


def deep_topk_window_dev(d_scores: int, d_rows: int, n: int, B: int, k: int, ascending: bool, row_offset: int, d_bounds: int,
                         d_out_ids: int, d_out_scores: int, d_scratch: int, stream: int = 0) -> None:
    """hr_deep_topk_window_dev: the first k of [B][n] candidates whose ranking key lies inside the query's open interval
    d_bounds [B][2] (uint64, device), by (score desc, row asc); scratch as deep_topk_dev at window k."""
    L = load_library()
    rc = L.hr_deep_topk_window_dev(_vp(d_scores), _vp(d_rows), n, B, k, 1 if ascending else 0, row_offset,
                                   _vp(d_bounds) if d_bounds else None, _vp(d_out_ids), _vp(d_out_scores), _vp(d_scratch),
                                   _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def deep_topk_scratch_bytes(n: int, B: int, window: int) -> int:
    """hr_deep_topk_scratch_bytes: device scratch hr_deep_topk_dev needs for B queries at offset + k = window."""
    return int(load_library().hr_deep_topk_scratch_bytes(n, B, window))


def deep_topk_dev(d_scores: int, d_rows: int, n: int, B: int, k: int, offset: int, ascending: bool, row_offset: int,
                  d_out_ids: int, d_out_scores: int, d_scratch: int, stream: int = 0):
    """hr_deep_topk_dev: entries offset .. offset + k - 1 of [B][n] candidates by (score desc, row asc), on device arrays."""
    L = load_library()
    rc = L.hr_deep_topk_dev(_vp(d_scores), _vp(d_rows), n, B, k, offset, 1 if ascending else 0, row_offset, _vp(d_out_ids),
                            _vp(d_out_scores), _vp(d_scratch), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def get_sparse_rows_scratch_bytes(n: int) -> int:
    """hr_get_sparse_rows_scratch_bytes: device scratch hr_get_sparse_rows_dev needs for n requested rows."""
    return int(load_library().hr_get_sparse_rows_scratch_bytes(n))


def mask_rows_dev(d_mask: int, n_rows: int, first_row: int, offset: int, limit: int, d_rows: int, d_counts: int,
                  d_scratch: int, stream: int = 0):
    """hr_mask_rows_dev: packed row mask (0 = every row) -> d_counts[0] = set bits below n_rows, d_counts[1] = ids written,
    d_rows[i] = first_row + the (offset + i)-th set bit (int64 device buffers; asynchronous on `stream`)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_mask_rows_dev(p(d_mask), n_rows, first_row, offset, limit, p(d_rows), p(d_counts), p(d_scratch), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def group_select_n_dev(d_ids: int, d_n: int, B: int, k_in: int, d_keys: int, key_rows: int, first_row: int, k_out: int,
                       group_size: int, d_out_pos: int, d_out_keys: int, d_out_cnt: int, d_out_n: int, d_flags: int, stream: int = 0):
    """hr_group_select_n_dev: the first group_size entries of every group of a batch of ranked lists (device pointers; 0 =
    NULL) -> positions [B][k_out * group_size], keys [B][k_out], members [B][k_out], groups [B], flags [B] (bit 0: the
    groups are final, bit 1: so are their members)."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_group_select_n_dev(p(d_ids), p(d_n), B, k_in, p(d_keys), key_rows, first_row, k_out, group_size, p(d_out_pos),
                                 p(d_out_keys), p(d_out_cnt), p(d_out_n), p(d_flags), p(stream))
    if rc != 0:
        _raise_global(L, rc)


def mask_keep_groups_dev(d_mask_in: int, d_mask_out: int, n_rows: int, d_keys: int, d_keep: int, n_keep: int, stream: int = 0):
    """hr_mask_keep_groups_dev: mask_out = mask_in (0 = all rows) restricted to the rows whose group key is among the n_keep keys."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_mask_keep_groups_dev(p(d_mask_in), p(d_mask_out), n_rows, p(d_keys), p(d_keep), n_keep, p(stream))
    if rc != 0:
        _raise_global(L, rc)


def mask_drop_groups_dev(d_mask_in: int, d_mask_out: int, n_rows: int, d_keys: int, d_drop: int, n_drop: int, stream: int = 0):
    """hr_mask_drop_groups_dev: mask_out = mask_in (0 = all rows) without the rows whose group key is among the n_drop keys."""
    L = load_library()
    p = lambda x: _vp(x) if x else None
    rc = L.hr_mask_drop_groups_dev(p(d_mask_in), p(d_mask_out), n_rows, p(d_keys), p(d_drop), n_drop, p(stream))
    if rc != 0:
        _raise_global(L, rc)


def merge_topk_dev(d_scores: int, d_ids: int, n_lists: int, B: int, k_in: int, k_out: int, d_out_ids: int,
                   d_out_scores: int, stream: int = 0, score_stride: int = 0, id_stride: int = 0, ascending: bool = False):
    """hr_merge_topk_dev, or with ascending=True hr_merge_topk_asc_dev (the distance lists of an L2 collection)."""
    L = load_library()
    rc = (L.hr_merge_topk_asc_dev if ascending else L.hr_merge_topk_dev)(_vp(d_scores), _vp(d_ids), n_lists, score_stride or B * k_in, id_stride or B * k_in, B,
                             k_in, k_out, _vp(d_out_ids), _vp(d_out_scores), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


class FilterTerm(ctypes.Structure):
    """hr_filter_term of include/hbmrag.h."""
    _fields_ = [("kind", _c.c_int32), ("op", _c.c_int32), ("col", _c.c_void_p), ("ival", _c.c_int64), ("dval", _c.c_double),
                ("fval", _c.c_float), ("reserved", _c.c_uint32), ("key", _c.c_uint64 * 2)]


HR_COL_I64, HR_COL_I64_VS_F64, HR_COL_F32, HR_COL_STR16 = 0, 1, 2, 3
FILTER_OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}


def filter_eval_dev(terms: Sequence["FilterTerm"], n_rows: int, d_deleted: int, d_mask: int, d_undecided: int,
                    d_counts: int, stream: int = 0):
    L = load_library()
    arr = (FilterTerm * max(len(terms), 1))(*terms)
    rc = L.hr_filter_eval_dev(ctypes.byref(arr), len(terms), n_rows, _vp(d_deleted) if d_deleted else None, _vp(d_mask),
                              _vp(d_undecided), _vp(d_counts), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


class FilterLeaf(ctypes.Structure):
    """hr_filter_leaf of include/hbmrag.h."""
    _fields_ = [("term", FilterTerm), ("set", _c.c_void_p), ("n_set", _c.c_int32), ("reserved", _c.c_int32)]


HR_OP_IN = 6
HR_COL_TOKENS, HR_OP_MATCH = 4, 7     # the keyword leaf (TEXT_MATCH): only together, only in hr_filter_eval_expr_dev
HR_FILTER_AND, HR_FILTER_OR, HR_FILTER_NOT = -1, -2, -3
HR_MAX_FILTER_TERMS, HR_MAX_FILTER_PROGRAM, HR_MAX_FILTER_SET_BYTES = 16, 64, 65536


def filter_eval_expr_dev(leaves: Sequence["FilterLeaf"], program: Sequence[int], n_rows: int, d_deleted: int, d_mask: int,
                         d_undecided: int, d_counts: int, stream: int = 0):
    """hr_filter_eval_expr_dev: leaves + postfix program -> packed row mask (include/hbmrag.h)."""
    L = load_library()
    arr = (FilterLeaf * max(len(leaves), 1))(*leaves)
    prog = (_c.c_int32 * max(len(program), 1))(*program)
    rc = L.hr_filter_eval_expr_dev(ctypes.byref(arr), len(leaves), ctypes.byref(prog), len(program), n_rows,
                                   _vp(d_deleted) if d_deleted else None, _vp(d_mask), _vp(d_undecided), _vp(d_counts),
                                   _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def bm25_encode_dev(d_text: int, d_off: int, n_docs: int, sparse_dim: int, k1: float, b: float, avgdl: float, cap: int,
                    d_idx: int, d_val: int, d_nnz: int, d_flags: int, stream: int = 0):
    """hr_bm25_encode_dev: BM25 document payloads of a batch on the device (include/hbmrag.h)."""
    L = load_library()
    rc = L.hr_bm25_encode_dev(_vp(d_text) if d_text else None, _vp(d_off), n_docs, sparse_dim, float(k1), float(b), float(avgdl), cap,
                              _vp(d_idx) if d_idx else None, _vp(d_val) if d_val else None, _vp(d_nnz), _vp(d_flags),
                              _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def hash_tokenize_dev(d_text: int, d_off: int, n: int, max_len: int, vocab: int, d_ids: int, d_lens: int, d_flags: int,
                      stream: int = 0):
    """hr_hash_tokenize_dev: the hash tokenizer of the encoder hooks for a batch of texts (include/hbmrag.h)."""
    L = load_library()
    rc = L.hr_hash_tokenize_dev(_vp(d_text) if d_text else None, _vp(d_off), n, max_len, vocab, _vp(d_ids) if d_ids else None,
                                _vp(d_lens), _vp(d_flags), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


class PostArgs(ctypes.Structure):
    """hr_post_args of include/hbmrag.h, field for field."""
    _fields_ = [
        ("ids", _c.c_void_p * 3), ("scores", _c.c_void_p * 3), ("k_in", _c.c_int32 * 3), ("k_fuse", _c.c_int32 * 3),
        ("n_lists", _c.c_int32), ("rrf_k", _c.c_int32), ("id_stride", _c.c_int64), ("score_stride", _c.c_int64),
        ("merged_ids", _c.c_void_p * 3), ("merged_scores", _c.c_void_p * 3), ("w", _c.c_double * 3),
        ("fused_ids", _c.c_void_p), ("fused_scores", _c.c_void_p), ("fused_methods", _c.c_void_p),
        ("fused_n", _c.c_void_p), ("top_k", _c.c_int32), ("rerank", _c.c_int32), ("base_w", _c.c_double),
        ("method_bonus", _c.c_double), ("recency_w", _c.c_double), ("recency", _c.c_void_p), ("k_out", _c.c_int32),
        ("asc_mask", _c.c_int32), ("rr_ids", _c.c_void_p), ("rr_scores", _c.c_void_p), ("rr_orig", _c.c_void_p),
        ("flags", _c.c_void_p), ("flag_stride", _c.c_int64), ("n_flag_rows", _c.c_int32), ("reserved2", _c.c_int32),
        ("agg_flags", _c.c_void_p), ("w_query", _c.c_void_p), ("fusion", _c.c_int32), ("norm", _c.c_int32 * 3),
    ]


def post_lists_dev(args: PostArgs, B: int, stream: int = 0):
    """[merge of every modality's exchanged lists] -> RRF -> [learned-ranker rerank] in one launch."""
    L = load_library()
    rc = L.hr_post_lists_dev(ctypes.byref(args), B, _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def debug_option(key: int, value: int):
    L = load_library()
    rc = L.hr_debug_option(None, key, value)
    if rc != 0:
        _raise_global(L, rc)


def stream_create(device: int = 0, priority: int = 0, cu_mask: Optional[Sequence[int]] = None) -> int:
    """A HIP stream (raw handle) with a priority or, when `cu_mask` (32-bit words, bit i = CU i) is given, confined to
    those compute units.  Wrap it with torch.cuda.ExternalStream; release it with stream_destroy."""
    L = load_library()
    out = ctypes.c_void_p()
    words = np.ascontiguousarray(cu_mask, dtype=np.uint32) if cu_mask is not None else None
    rc = L.hr_stream_create(device, priority, _vp(words) if words is not None else None,
                            0 if words is None else int(words.shape[0]), ctypes.byref(out))
    if rc != 0:
        _raise_global(L, rc)
    return int(out.value)


def stream_destroy(device: int, stream: int):
    L = load_library()
    rc = L.hr_stream_destroy(device, _vp(stream))
    if rc != 0:
        _raise_global(L, rc)


def cu_mask_words(n_cus_total: int, lo: int, hi: int):
    """32-bit mask words with bits [lo, hi) set out of n_cus_total."""
    words = np.zeros((n_cus_total + 31) // 32, dtype=np.uint32)
    for i in range(lo, hi):
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return words


def add_layernorm_f16_dev(d_x: int, d_residual: int, d_gamma: int, d_beta: int, d_out: int, rows: int, hidden: int,
                          eps: float, stream: int = 0):
    """out = LayerNorm(x (+ residual)) * gamma + beta over fp16 rows (device pointers; d_residual may be 0)."""
    L = load_library()
    rc = L.hr_add_layernorm_f16_dev(_vp(d_x), _vp(d_residual) if d_residual else None, _vp(d_gamma), _vp(d_beta),
                                    _vp(d_out), rows, hidden, eps, _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def embed_layernorm_f16_dev(d_ids: int, d_types: int, d_word: int, d_pos: int, d_seg: int, d_gamma: int, d_beta: int, d_out: int,
                            n_seq: int, T: int, hidden: int, eps: float, n_word: int, n_seg: int, stream: int = 0):
    """out[s, t] = LayerNorm(word[ids[s, t]] + pos[t] + seg[types[s, t]]): int64 ids / types (clamped into the tables),
    fp16 tables and output."""
    L = load_library()
    rc = L.hr_embed_layernorm_f16_dev(_vp(d_ids), _vp(d_types), _vp(d_word), _vp(d_pos), _vp(d_seg), _vp(d_gamma), _vp(d_beta),
                                      _vp(d_out), n_seq, T, hidden, float(eps), n_word, n_seg, _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def attention_f16_dev(d_qkv: int, d_lengths: int, d_out: int, n_seq: int, T: int, heads: int, head_dim: int, scale: float,
                      stream: int = 0):
    """softmax(scale Q K^T) V per head from a fused [n_seq, T, 3, heads, head_dim] fp16 QKV buffer into [n_seq, T, H]."""
    L = load_library()
    rc = L.hr_attention_f16_dev(_vp(d_qkv), _vp(d_lengths) if d_lengths else None, _vp(d_out), n_seq, T, heads, head_dim,
                                float(scale), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def linear_rows_f16_dev(d_x: int, x_fr: bool, d_w_packed: int, d_bias: int, d_out: int, rows: int, K: int, N: int, out_stride: int,
                        stream: int = 0):
    """out[r][:N] = x[r][:K] W^T + bias through the hand-written MFMA kernel (x row-major with naturally packed weights, or
    in fragment order with weights in accumulator k order: encoder_kernels.pack_natural / pack_accumulator_order)."""
    L = load_library()
    rc = L.hr_linear_rows_f16_dev(_vp(d_x), 1 if x_fr else 0, _vp(d_w_packed), _vp(d_bias), _vp(d_out), rows, K, N, out_stride,
                                  _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def attention_fr_f16_dev(d_qkv: int, d_lengths: int, d_out_fr: int, n_seq: int, T: int, heads: int, head_dim: int, scale: float,
                         stream: int = 0):
    """hr_attention_f16_dev with its output in fragment order (what hr_encoder_tail_f16_dev reads)."""
    L = load_library()
    rc = L.hr_attention_fr_f16_dev(_vp(d_qkv), _vp(d_lengths) if d_lengths else None, _vp(d_out_fr), n_seq, T, heads, head_dim,
                                   float(scale), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def encoder_tail_f16_dev(d_attn_fr: int, d_x: int, x_fr: bool, d_out: int, out_fr: bool, d_wstream: int, d_tables: int, rows: int,
                         hidden: int, intermediate: int, eps: float, gelu_erf: bool, stream: int = 0):
    """Everything of a post-LN layer after the attention in one launch (csrc/encoder_layer.h)."""
    L = load_library()
    rc = L.hr_encoder_tail_f16_dev(_vp(d_attn_fr), _vp(d_x), 1 if x_fr else 0, _vp(d_out), 1 if out_fr else 0, _vp(d_wstream),
                                   _vp(d_tables), rows, hidden, intermediate, float(eps), 1 if gelu_erf else 0,
                                   _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def attention_rows_f16_dev(d_q: int, q_seq_stride: int, q_token_stride: int, d_k: int, d_v: int, kv_seq_stride: int,
                           kv_token_stride: int, d_lengths: int, d_out: int, n_seq: int, T: int, n_queries: int, heads: int,
                           head_dim: int, scale: float, stream: int = 0):
    """The attention kernel with operands by pointer and stride (halves): the first n_queries tokens are the queries."""
    L = load_library()
    rc = L.hr_attention_rows_f16_dev(_vp(d_q), q_seq_stride, q_token_stride, _vp(d_k), _vp(d_v), kv_seq_stride, kv_token_stride,
                                     _vp(d_lengths) if d_lengths else None, _vp(d_out), n_seq, T, n_queries, heads, head_dim,
                                     float(scale), _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)


def rerank_linear_dev(d_ids: int, d_scores: int, d_methods: int, d_n: int, B: int, k_in: int, base_w: float,
                      method_bonus: float, recency_w: float, k_out: int, d_out_ids: int, d_out_scores: int,
                      d_out_orig: int, stream: int = 0, d_recency: int = 0):
    L = load_library()
    rc = L.hr_rerank_linear_dev(_vp(d_ids), _vp(d_scores), _vp(d_methods), _vp(d_n),
                                _vp(d_recency) if d_recency else None, B, k_in, base_w, method_bonus, recency_w,
                                k_out, _vp(d_out_ids), _vp(d_out_scores), _vp(d_out_orig),
                                _vp(stream) if stream else None)
    if rc != 0:
        _raise_global(L, rc)
