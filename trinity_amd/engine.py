"""ctypes harness over the C-ABI (include/trinity_hip.h) and the host tools (csrc/host/synth.cpp).

No fallbacks: a missing libtrinity_hip.so, a missing GPU or a failing call raises TrinityError."""
import collections
import ctypes as C
import os

import numpy as np

from .build import LIB_HIP, LIB_HOST

# perf probes: an alternative build of the engine (build/libtrinity_hip_*.so: -DTRI_PROF, other launch bounds ...) for this process.
# The harness only — the library itself reads nothing from the environment.
LIB_HIP = os.environ.get("TRINITY_HIP_LIB") or LIB_HIP
LIB_HOST = os.environ.get("TRINITY_HOST_LIB") or LIB_HOST  # (the host tools under ThreadSanitizer: tests/test_planner_tsan.py)

OP_TERM, OP_AND, OP_OR, OP_PHRASE, OP_NOT, OP_OPT, OP_SOME = 0, 1, 2, 3, 4, 5, 6  # OP_SOME: arg = (min << 16) | children (matchsome)
FLAG_DOCUMENTS_ONLY, FLAG_ACCUMULATED_SCORE, FLAG_MATCHED_TERMS, FLAG_HIT_PAYLOADS = 1, 2, 4, 8
CODEC_GOOGLE, CODEC_LUCENE = 1, 2
FNV_EMPTY = 1469598103934665603


class TrinityError(RuntimeError):
    pass


def tok(op, arg):
    return (op << 28) | (arg & 0x0FFFFFFF)


class TriTerm(C.Structure):
    _fields_ = [("documents", C.c_uint32), ("offset", C.c_uint32), ("size", C.c_uint32)]


class TriQuery(C.Structure):
    _fields_ = [("prog_off", C.c_uint32), ("prog_len", C.c_uint32)]


class TriRanker(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("topk", C.c_uint32), ("freq_cap", C.c_uint32), ("reserved", C.c_uint32), ("adjacency", C.c_double)]


RANK_PROXIMITY = 1


class TriFacet(C.Structure):
    _fields_ = [("column", C.c_void_p), ("nbuckets", C.c_uint32), ("reserved", C.c_uint32)]


class TriOrder(C.Structure):
    _fields_ = [("column", C.c_void_p), ("topk", C.c_uint32), ("descending", C.c_uint32), ("reserved", C.c_uint32)]


class TriStat(C.Structure):
    _fields_ = [("group", C.c_void_p), ("value", C.c_void_p), ("nbuckets", C.c_uint32), ("reserved", C.c_uint32)]


class TriClause(C.Structure):
    _fields_ = [("column", C.c_void_p), ("kind", C.c_uint32), ("negate", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("set", C.c_void_p), ("nset", C.c_uint32),
                ("reserved", C.c_uint32)]  # fmt: skip


class TriPredicate(C.Structure):
    _fields_ = [("clauses", C.POINTER(TriClause)), ("nclauses", C.c_uint32), ("any", C.c_uint32), ("also", C.c_void_p), ("reserved", C.c_uint64)]


class TriIsectRequest(C.Structure):
    _fields_ = [("ngroups", C.c_uint32), ("reserved", C.c_uint32), ("stopwords_mask", C.c_uint64)]


class TriIsectInfo(C.Structure):
    _fields_ = [("span_docs", C.c_uint32), ("lds_slots", C.c_uint32), ("nreq", C.c_uint32), ("nspans", C.c_uint32), ("rows", C.c_uint32), ("max_masks", C.c_uint32),
                ("max_runs", C.c_uint32), ("passes", C.c_uint32), ("row_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64), ("h_size", C.POINTER(C.c_uint32)),
                ("c_size", C.POINTER(C.c_uint32)), ("lds_spills", C.POINTER(C.c_uint32))]  # fmt: skip


class TriPercDocs(C.Structure):
    _fields_ = [("ndocs", C.c_uint32), ("doc_first", C.c_void_p), ("terms", C.c_void_p), ("freqs", C.c_void_p), ("positions", C.c_void_p), ("npositions", C.c_uint64),
                ("reserved", C.c_uint32)]  # fmt: skip


class TriPercInfo(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("unsupported", C.c_uint64), ("terms", C.c_uint64), ("phrases", C.c_uint64), ("device_bytes", C.c_uint64), ("nterms", C.c_uint32),
                ("reserved", C.c_uint32)]  # fmt: skip


class TriPercResultInfo(C.Structure):
    _fields_ = [("ndocs", C.c_uint32), ("leaf_rows", C.c_uint32), ("phrase_rows", C.c_uint32), ("evaluated", C.c_uint32), ("hit_queries", C.c_uint32), ("reserved", C.c_uint32),
                ("pairs", C.c_uint64), ("scratch_bytes", C.c_uint64), ("rows_ms", C.c_float), ("phrases_ms", C.c_float), ("select_ms", C.c_float), ("eval_ms", C.c_float),
                ("compact_ms", C.c_float), ("total_ms", C.c_float)]  # fmt: skip


PERC_BY_QUERY, PERC_BY_DOCUMENT = 0, 1
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


class TriIndexInfo(C.Structure):
    _fields_ = [
        ("index_bytes", C.c_uint64),
        ("directory_bytes", C.c_uint64),
        ("blocks", C.c_uint64),
        ("postings", C.c_uint64),
        ("doc_bytes", C.c_uint64),
        ("hit_bytes", C.c_uint64),
        ("nterms", C.c_uint32),
        ("docs_cnt", C.c_uint32),
    ]


class TriBatchInfo(C.Structure):
    _fields_ = [
        ("nqueries", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("matches", C.c_uint64),
        ("out_capacity", C.c_uint64),
        ("last_run_ms", C.c_float),
        ("launches", C.c_uint32),
        ("dense_ms", C.c_float),
        ("cand_ms", C.c_float),
        ("dense_algorithmic_bytes", C.c_uint64),
        ("cand_algorithmic_bytes", C.c_uint64),
        ("dense_queries", C.c_uint64),
        ("cand_queries", C.c_uint64),
        ("fused_ms", C.c_float),
        ("rest_ms", C.c_float),
        ("fused_algorithmic_bytes", C.c_uint64),
        ("fused_queries", C.c_uint64),
        ("cand_needed_bytes", C.c_uint64),
        ("phrase_ms", C.c_float),
        ("tree_ms", C.c_float),
        ("phrase_algorithmic_bytes", C.c_uint64),
        ("phrase_queries", C.c_uint64),
        ("term_planes_ms", C.c_float),
        ("planes_ms", C.c_float),
        ("planes_algorithmic_bytes", C.c_uint64),
        ("planes_queries", C.c_uint64),
        ("plane_terms", C.c_uint64),
        ("plane_bytes", C.c_uint64),
        ("term_planes_decoded_bytes", C.c_uint64),
        ("unsupported_queries", C.c_uint64),
        ("create_ms", C.c_float),
        ("create_plan_ms", C.c_float),
        ("bound_bytes", C.c_uint64),
        ("dense_bound_bytes", C.c_uint64),
        ("cand_bound_bytes", C.c_uint64),
        ("fused_bound_bytes", C.c_uint64),
        ("planes_bound_bytes", C.c_uint64),
        ("phrase_bound_bytes", C.c_uint64),
        ("pset_ms", C.c_float),
        ("probe_ms", C.c_float),
        ("pset_queries", C.c_uint64),
        ("pset_algorithmic_bytes", C.c_uint64),
        ("pset_bound_bytes", C.c_uint64),
        ("probe_queries", C.c_uint64),
        ("probe_algorithmic_bytes", C.c_uint64),
        ("probe_bound_bytes", C.c_uint64),
        ("tree_queries", C.c_uint64),
        ("tree_scratch_bytes", C.c_uint64),
        ("bitmap_queries", C.c_uint64),
    ]


# every symbol include/trinity_hip.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = [
    "tri_last_error", "tri_abi_version", "tri_dev_open", "tri_dev_close", "tri_dev_sync", "tri_dev_stream", "tri_dev_set_option", "tri_dev_get_option", "tri_dev_memory",
    "tri_index_upload", "tri_index_destroy", "tri_index_get_info", "tri_index_term_docbytes", "tri_index_set_masked", "tri_decode_terms", "tri_decode_hits", "tri_decode_hits_at",
    "tri_batch_create", "tri_batch_query_status", "tri_batch_destroy", "tri_batch_run", "tri_batch_sync", "tri_batch_get_info",
    "tri_batch_match_counts", "tri_batch_docset", "tri_batch_docset_bitmap", "tri_batch_docsets", "tri_batch_docsets_mixed", "tri_batch_scores", "tri_batch_query_terms", "tri_batch_matched_terms", "tri_batch_query_terms_wide", "tri_batch_matched_terms_wide", "tri_batch_matched_payloads", "tri_batch_set_ranker", "tri_batch_ranked", "tri_batch_topk", "tri_batch_topk_device", "tri_batch_counts_device", "tri_batch_docset_hashes",
    "tri_cbatch_create", "tri_cbatch_destroy", "tri_cbatch_query_status", "tri_cbatch_run", "tri_cbatch_sync", "tri_cbatch_match_counts", "tri_cbatch_topk", "tri_cbatch_docset", "tri_cbatch_ranked", "tri_cbatch_matched_terms", "tri_cbatch_matched_terms_wide", "tri_cbatch_matched_payloads", "tri_encode_google", "tri_encode_google_payloads", "tri_commit_google", "tri_commit_lucene", "tri_merge_google", "tri_merge_lucene", "tri_encode_lucene", "tri_encode_lucene_payloads", "tri_commit_lucene_payloads",
    "tri_comm_unique_id", "tri_comm_create", "tri_comm_create_custom", "tri_comm_destroy", "tri_gather_results",
    "tri_filter_create", "tri_filter_from_docset", "tri_filter_destroy", "tri_batch_set_filters",
    "tri_isect_run", "tri_isect_status", "tri_isect_results", "tri_isect_histogram", "tri_isect_get_info", "tri_isect_destroy",
    "tri_perc_create", "tri_perc_query_status", "tri_perc_set_enabled", "tri_perc_get_info", "tri_perc_destroy", "tri_perc_match",
    "tri_perc_result_pairs", "tri_perc_result_doc_counts", "tri_perc_result_get_info", "tri_perc_result_destroy",
    "tri_column_create", "tri_column_destroy", "tri_batch_set_facets", "tri_batch_facets", "tri_cbatch_facets",
    "tri_batch_set_order", "tri_batch_ordered", "tri_cbatch_ordered",
    "tri_batch_set_stats", "tri_batch_stats", "tri_cbatch_stats",
    "tri_filters_from_columns", "tri_filter_bitmap",
]  # fmt: skip

_hip = None
_host = None


def hip_lib():
    """Load libtrinity_hip.so; raises (never falls back) when it is missing."""
    global _hip
    if _hip is not None:
        return _hip
    if not os.path.exists(LIB_HIP):
        raise TrinityError(f"{LIB_HIP} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` — there is no CPU fallback")
    L = C.CDLL(LIB_HIP)
    vp, u32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.tri_last_error.restype = C.c_char_p
    L.tri_abi_version.restype = C.c_int
    L.tri_dev_open.argtypes = [C.c_int, C.POINTER(vp)]
    L.tri_dev_close.argtypes = [vp]
    L.tri_dev_sync.argtypes = [vp]
    L.tri_dev_stream.restype = vp
    L.tri_dev_stream.argtypes = [vp]
    L.tri_dev_set_option.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.tri_dev_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]
    L.tri_dev_memory.argtypes = [vp, C.POINTER(C.c_uint64 * 5)]
    L.tri_index_upload.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_uint32, C.POINTER(vp)]
    L.tri_index_destroy.argtypes = [vp]
    L.tri_index_get_info.argtypes = [vp, C.POINTER(TriIndexInfo)]
    L.tri_index_term_docbytes.argtypes = [vp, vp, C.c_size_t, vp]
    L.tri_index_set_masked.argtypes = [vp, vp, C.c_size_t]
    L.tri_decode_terms.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    L.tri_decode_hits.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
    L.tri_decode_hits_at.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t, vp]
    L.tri_batch_create.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.tri_batch_query_status.argtypes = [vp, vp]
    L.tri_batch_destroy.argtypes = [vp]
    L.tri_batch_run.argtypes = [vp]
    L.tri_batch_sync.argtypes = [vp]
    L.tri_batch_get_info.argtypes = [vp, C.POINTER(TriBatchInfo)]
    L.tri_batch_query_terms.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_uint32)]
    L.tri_batch_matched_terms.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_batch_query_terms_wide.argtypes = L.tri_batch_query_terms.argtypes
    L.tri_batch_matched_terms_wide.argtypes = L.tri_batch_matched_terms.argtypes
    L.tri_batch_matched_payloads.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_batch_match_counts.argtypes = [vp, vp]
    L.tri_batch_docset.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_batch_docsets.argtypes = [vp, vp, C.c_size_t, vp]
    L.tri_batch_docsets_mixed.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.tri_batch_docset_bitmap.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int), vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
    L.tri_batch_scores.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_batch_topk.argtypes = [vp, vp, vp, vp]
    L.tri_batch_topk_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.tri_batch_counts_device.argtypes = [vp, C.POINTER(vp)]
    L.tri_batch_docset_hashes.argtypes = [vp, vp]
    L.tri_cbatch_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.tri_cbatch_destroy.argtypes = [vp]
    L.tri_cbatch_query_status.argtypes = [vp, vp]
    L.tri_cbatch_run.argtypes = [vp]
    L.tri_cbatch_sync.argtypes = [vp]
    L.tri_cbatch_match_counts.argtypes = [vp, vp]
    L.tri_cbatch_topk.argtypes = [vp, vp, vp, vp]
    L.tri_cbatch_docset.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_cbatch_ranked.argtypes = [vp, vp, vp, vp]
    L.tri_cbatch_matched_terms.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_cbatch_matched_terms_wide.argtypes = L.tri_cbatch_matched_terms.argtypes
    L.tri_cbatch_matched_payloads.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_encode_google.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_encode_google_payloads.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_encode_lucene.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_commit_lucene.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, C.c_size_t,
                                    C.POINTER(C.c_size_t), vp]
    L.tri_encode_lucene_payloads.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_commit_lucene_payloads.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp,
                                             C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_merge_google.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp]
    L.tri_merge_lucene.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp]
    L.tri_commit_google.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.tri_comm_unique_id.argtypes = [vp]
    L.tri_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.tri_comm_create_custom.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
    L.tri_comm_destroy.argtypes = [vp]
    L.tri_gather_results.argtypes = [vp, vp, vp, vp, vp, vp]
    L.tri_filter_create.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.tri_filter_from_docset.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.tri_filter_destroy.argtypes = [vp]
    L.tri_filter_destroy.restype = None
    L.tri_batch_set_filters.argtypes = [vp, vp, C.c_size_t, vp]
    L.tri_filters_from_columns.argtypes = [vp, C.POINTER(TriPredicate), C.c_size_t, C.c_int, C.POINTER(vp)]
    L.tri_filter_bitmap.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_batch_set_ranker.argtypes = [vp, vp, vp]
    L.tri_column_create.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.tri_column_destroy.argtypes = [vp]
    L.tri_column_destroy.restype = None
    L.tri_batch_set_facets.argtypes = [vp, C.POINTER(TriFacet), C.c_size_t]
    L.tri_batch_facets.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
    L.tri_cbatch_facets.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
    L.tri_batch_set_order.argtypes = [vp, C.POINTER(TriOrder)]
    L.tri_batch_ordered.argtypes = [vp, vp, vp, vp]
    L.tri_cbatch_ordered.argtypes = [vp, vp, vp, vp]
    L.tri_batch_set_stats.argtypes = [vp, C.POINTER(TriStat), C.c_size_t]
    L.tri_batch_stats.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
    L.tri_cbatch_stats.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
    L.tri_isect_run.argtypes = [vp, vp, C.c_size_t, vp, vp, C.POINTER(vp)]
    L.tri_isect_status.argtypes = [vp, vp]
    L.tri_isect_results.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_isect_histogram.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_isect_get_info.argtypes = [vp, C.POINTER(TriIsectInfo)]
    L.tri_isect_destroy.argtypes = [vp]
    L.tri_isect_destroy.restype = None
    L.tri_batch_ranked.argtypes = [vp, vp, vp, vp]
    L.tri_perc_create.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.POINTER(vp)]
    L.tri_perc_query_status.argtypes = [vp, vp]
    L.tri_perc_set_enabled.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.tri_perc_get_info.argtypes = [vp, C.POINTER(TriPercInfo)]
    L.tri_perc_destroy.argtypes = [vp]
    L.tri_perc_destroy.restype = None
    L.tri_perc_match.argtypes = [vp, C.POINTER(TriPercDocs), C.POINTER(vp)]
    L.tri_perc_result_pairs.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tri_perc_result_doc_counts.argtypes = [vp, vp]
    L.tri_perc_result_get_info.argtypes = [vp, C.POINTER(TriPercResultInfo)]
    L.tri_perc_result_destroy.argtypes = [vp]
    L.tri_perc_result_destroy.restype = None
    _hip = L
    return L


def host_lib():
    global _host
    if _host is not None:
        return _host
    if not os.path.exists(LIB_HOST):
        raise TrinityError(f"{LIB_HOST} is missing: run __graft_entry__.build()")
    L = C.CDLL(LIB_HOST)
    L.tri_synth_segment_build.restype = C.c_void_p
    L.tri_synth_segment_build.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    L.tri_synth_segment_build_codec.restype = C.c_void_p
    L.tri_synth_segment_build_codec.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int]
    L.tri_synth_segment_hits.restype = C.POINTER(C.c_uint8)
    L.tri_synth_segment_hits.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.tri_synth_segment_free.argtypes = [C.c_void_p]
    L.tri_host_encode_google.restype = C.c_longlong
    L.tri_host_encode_google.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.tri_host_encode_google_payloads.restype = C.c_longlong
    L.tri_host_encode_google_payloads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.tri_synth_segment_index.restype = C.POINTER(C.c_uint8)
    L.tri_synth_segment_index.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.tri_synth_segment_terms.restype = C.POINTER(C.c_uint32)
    L.tri_synth_segment_terms.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.tri_synth_segment_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.tri_synth_queries.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.tri_host_perc_lower.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64]
    L.tri_host_perc_check_docs.argtypes = [C.POINTER(TriPercDocs), C.c_uint32, C.c_char_p, C.c_uint64]
    _host = L
    return L


def _check(rc):
    if rc != 0:
        raise TrinityError(f"rc={rc}: {hip_lib().tri_last_error().decode()}")


def _size_then_fill(call, lens, nterms=None):
    """The write side's size-then-fill protocol.  call(out, cap, ...) takes a (byte buffer, capacity) pair per length of `lens` (c_size_t: the index, then
    hits.data where the codec has one) and, when `nterms` (c_size_t) is given, (termIDs, term table, their capacity) after them.  Called with null outputs it
    leaves the lengths; the outputs are allocated from those, the call is repeated, and the outputs come back cut to their lengths."""
    _check(call(*[None, 0] * len(lens), *([None, None, 0] if nterms is not None else [])))
    bufs = [np.zeros(max(1, n.value), dtype=np.uint8) for n in lens]
    args = [x for b in bufs for x in (b.ctypes.data, b.size)]
    outs = [b[: n.value] for b, n in zip(bufs, lens)]
    if nterms is not None:
        tids, terms = np.zeros(max(1, nterms.value), dtype=np.uint32), np.zeros((max(1, nterms.value), 3), dtype=np.uint32)
        args += [tids.ctypes.data, terms.ctypes.data, nterms.value]
        outs += [tids[: nterms.value], terms[: nterms.value]]
    _check(call(*args))
    return outs


def _commit_stats(arr):
    """tri_commit_stats as a dict"""
    return dict(zip(("docs_cnt", "sum_terms_docs", "sum_term_hits", "total_terms"), (int(x) for x in arr)))


def gen_queries(V, seed, nq, nterms):
    out = np.zeros((nq, nterms), dtype=np.uint32)
    host_lib().tri_synth_queries(V, seed, nq, nterms, out.ctypes.data)
    return out


def gen_phrase_queries(D, V, slots, corpus_seed, seed, nq, nterms):
    """cfg4 phrases: even rows are consecutive tokens of a random document (>= 1 match), odd rows random Zipf terms."""
    out = np.zeros((nq, nterms), dtype=np.uint32)
    L = host_lib()
    L.tri_synth_phrase_queries.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.tri_synth_phrase_queries.restype = None
    L.tri_synth_phrase_queries(D, V, slots, corpus_seed, seed, nq, nterms, out.ctypes.data)
    return out


def flatten(programs):
    """(flat u32 program, (nq, 2) u32 tri_query table of (offset, length)) of a list of postfix programs — laid out with numpy (a ctypes
    struct array costs a microsecond per field store)."""
    progs = [np.ascontiguousarray(p, dtype=np.uint32) for p in programs]
    flat = np.concatenate(progs) if progs else np.zeros(0, np.uint32)
    q = np.zeros((max(1, len(progs)), 2), dtype=np.uint32)
    if progs:
        q[:, 1] = np.fromiter((p.size for p in progs), dtype=np.uint32, count=len(progs))
        q[1:, 0] = np.cumsum(q[:-1, 1], dtype=np.uint64).astype(np.uint32)
    return flat, q


class Segment:
    """A synthetic GOOGLE-codec segment built on the host (csrc/host/synth.cpp): raw `index` bytes + term table."""

    def __init__(self, D, V, slots=10, seed=42, codec=CODEC_GOOGLE):
        L = host_lib()
        # codec 3: the LUCENE-shaped container with FastPFor<4> payload words (what the reference's own build writes; csrc/fastpfor128.hpp) —
        # to everything downstream it is a LUCENE segment (codec 2)
        self.D, self.V, self.slots, self.seed, self.codec, self.payload = D, V, slots, seed, min(codec, CODEC_LUCENE), "fastpfor" if codec == 3 else "native"
        self.h = L.tri_synth_segment_build_codec(D, V, slots, seed, codec)
        if not self.h:
            raise TrinityError("segment build failed (index larger than 4 GiB?)")
        n = C.c_uint64()
        p = L.tri_synth_segment_index(self.h, C.byref(n))
        self.index = np.ctypeslib.as_array(p, shape=(n.value,))
        hp = L.tri_synth_segment_hits(self.h, C.byref(n))
        self.hits = np.ctypeslib.as_array(hp, shape=(n.value,)) if n.value else np.zeros(0, np.uint8)
        nt = C.c_uint32()
        tp = L.tri_synth_segment_terms(self.h, C.byref(nt))
        self.terms = np.ctypeslib.as_array(tp, shape=(nt.value, 3))
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        L.tri_synth_segment_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self.sum_terms_docs, self.sum_term_hits, self.total_terms, self.docs_cnt = a.value, b.value, c.value, d.value

    def __del__(self):
        try:
            if self.h:
                host_lib().tri_synth_segment_free(self.h)
                self.h = None
        except Exception:
            pass


class Device:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(hip_lib().tri_dev_open(device, C.byref(self.h)))

    def sync(self):
        _check(hip_lib().tri_dev_sync(self.h))

    def set_option(self, name, value):
        """Planner / launch option (include/trinity_hip.h tri_dev_set_option); applies to batches created afterwards."""
        _check(hip_lib().tri_dev_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_uint64()
        _check(hip_lib().tri_dev_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def memory(self):
        """tri_dev_memory: the handle's buffer pool (in use / idle), its idle pinned blocks, and the device's free / total bytes."""
        v = (C.c_uint64 * 5)()
        _check(hip_lib().tri_dev_memory(self.h, C.byref(v)))
        return dict(zip(("pool_in_use_bytes", "pool_idle_bytes", "pinned_idle_bytes", "device_free_bytes", "device_total_bytes"), (int(x) for x in v)))

    def encode_google(self, docs, freqs, positions, term_first, payload_lens=None, payloads=None):
        """The write side on the device (tri_encode_google / tri_encode_google_payloads): postings of len(term_first) - 1 terms ->
        (index bytes u8[], term table u32[n, 3]).  payload_lens / payloads: per hit, its payload's length (0 .. 8) and bytes (u64, first byte low)."""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        p = np.ascontiguousarray(positions, dtype=np.uint16)
        tf = np.ascontiguousarray(term_first, dtype=np.uint64)
        n = tf.size - 1
        terms = np.zeros((max(n, 1), 3), dtype=np.uint32)
        ln = C.c_size_t()
        L = hip_lib()
        if payload_lens is None:
            call = lambda out, cap: L.tri_encode_google(self.h, d.ctypes.data, f.ctypes.data, p.ctypes.data, p.size, tf.ctypes.data, n, out, cap, C.byref(ln), terms.ctypes.data)
        else:
            pl = np.ascontiguousarray(payload_lens, dtype=np.uint8)
            pv = np.ascontiguousarray(payloads, dtype=np.uint64)
            assert pl.size == p.size == pv.size
            call = lambda out, cap: L.tri_encode_google_payloads(self.h, d.ctypes.data, f.ctypes.data, p.ctypes.data, pl.ctypes.data, pv.ctypes.data, p.size, tf.ctypes.data, n, out,
                                                                  cap, C.byref(ln), terms.ctypes.data)  # fmt: skip
        (out,) = _size_then_fill(call, [ln])
        return out, terms[:n]

    def commit_google(self, term_ids, doc_ids, freqs, positions, payload_lens=None, payloads=None):
        """SegmentIndexSession::commit on the device (tri_commit_google): a session's postings in insertion order -> (index bytes u8[], the committed
        termIDs u32[n] in commit order, their term table u32[n, 3], stats {docs_cnt, sum_terms_docs, sum_term_hits, total_terms})."""
        t = np.ascontiguousarray(term_ids, dtype=np.uint32)
        d = np.ascontiguousarray(doc_ids, dtype=np.uint32)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        p = np.ascontiguousarray(positions, dtype=np.uint16)
        pl = None if payload_lens is None else np.ascontiguousarray(payload_lens, dtype=np.uint8)
        pv = None if payload_lens is None else np.ascontiguousarray(payloads, dtype=np.uint64)
        assert t.size == d.size == f.size and (pl is None or pl.size == p.size == pv.size)
        ln, nt = C.c_size_t(), C.c_size_t()
        stats = np.zeros(4, dtype=np.uint64)
        L = hip_lib()

        def call(out, cap, tids, terms, tcap):
            return L.tri_commit_google(self.h, t.ctypes.data, d.ctypes.data, f.ctypes.data, p.ctypes.data, None if pl is None else pl.ctypes.data,
                                       None if pv is None else pv.ctypes.data, t.size, p.size, out, cap, C.byref(ln), tids, terms, tcap, C.byref(nt), stats.ctypes.data)  # fmt: skip

        out, tids, terms = _size_then_fill(call, [ln], nt)
        return out, tids, terms, _commit_stats(stats)

    def commit_lucene(self, term_ids, doc_ids, freqs, positions, payload_lens=None, payloads=None):
        """tri_commit_lucene / tri_commit_lucene_payloads: a session's postings in insertion order -> (index bytes, hits.data bytes, committed termIDs, term table, stats).
        payload_lens / payloads: per hit, its payload's length (0 .. 8) and bytes (u64, first byte low); None: the payload-less export."""
        t = np.ascontiguousarray(term_ids, dtype=np.uint32)
        d = np.ascontiguousarray(doc_ids, dtype=np.uint32)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        p = np.ascontiguousarray(positions, dtype=np.uint16)
        pl = None if payload_lens is None else np.ascontiguousarray(payload_lens, dtype=np.uint8)
        pv = None if payloads is None else np.ascontiguousarray(payloads, dtype=np.uint64)
        assert t.size == d.size == f.size and (pl is None or pl.size == p.size) and (pv is None or pv.size == p.size)
        il, hl, nt = C.c_size_t(), C.c_size_t(), C.c_size_t()
        stats = np.zeros(4, dtype=np.uint64)
        L = hip_lib()

        def call(io, ic, ho, hc, tids, terms, tcap):
            if pl is None and pv is None:
                return L.tri_commit_lucene(self.h, t.ctypes.data, d.ctypes.data, f.ctypes.data, p.ctypes.data, t.size, p.size, io, ic, C.byref(il), ho, hc, C.byref(hl), tids, terms,
                                           tcap, C.byref(nt), stats.ctypes.data)  # fmt: skip
            return L.tri_commit_lucene_payloads(self.h, t.ctypes.data, d.ctypes.data, f.ctypes.data, p.ctypes.data, None if pl is None else pl.ctypes.data,
                                                None if pv is None else pv.ctypes.data, t.size, p.size, io, ic, C.byref(il), ho, hc, C.byref(hl), tids, terms, tcap, C.byref(nt),
                                                stats.ctypes.data)  # fmt: skip

        io, ho, tids, terms = _size_then_fill(call, [il, hl], nt)
        return io, ho, tids, terms, _commit_stats(stats)

    def encode_lucene(self, docs, freqs, positions, term_first, payload_lens=None, payloads=None):
        """The Lucene-shaped codec's encoder on the device (tri_encode_lucene / tri_encode_lucene_payloads, PFOR128 payload): -> (index bytes, hits.data bytes, term table
        u32[n, 3]).  payload_lens / payloads: per hit, its payload's length (0 .. 8) and bytes (u64, first byte low); None: the payload-less export."""
        d = np.ascontiguousarray(docs, dtype=np.uint32)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        p = np.ascontiguousarray(positions, dtype=np.uint16)
        tf = np.ascontiguousarray(term_first, dtype=np.uint64)
        n = tf.size - 1
        terms = np.zeros((max(n, 1), 3), dtype=np.uint32)
        il, hl = C.c_size_t(), C.c_size_t()
        L = hip_lib()
        if payload_lens is None and payloads is None:
            call = lambda io, ic, ho, hc: L.tri_encode_lucene(self.h, d.ctypes.data, f.ctypes.data, p.ctypes.data, p.size, tf.ctypes.data, n, io, ic, C.byref(il), ho, hc, C.byref(hl), terms.ctypes.data)
        else:
            pl = None if payload_lens is None else np.ascontiguousarray(payload_lens, dtype=np.uint8)
            pv = None if payloads is None else np.ascontiguousarray(payloads, dtype=np.uint64)
            assert (pl is None or pl.size == p.size) and (pv is None or pv.size == p.size)
            call = lambda io, ic, ho, hc: L.tri_encode_lucene_payloads(self.h, d.ctypes.data, f.ctypes.data, p.ctypes.data, None if pl is None else pl.ctypes.data,
                                                                        None if pv is None else pv.ctypes.data, p.size, tf.ctypes.data, n, io, ic, C.byref(il), ho, hc, C.byref(hl),
                                                                        terms.ctypes.data)  # fmt: skip
        io, ho = _size_then_fill(call, [il, hl])
        return io, ho, terms[:n]

    def merge_google(self, parts, part_terms):
        """Codecs::Google::IndexSession::merge for a whole dictionary (tri_merge_google): parts = uploaded google_codec Index objects, most recent first
        (each with its masked documents set); part_terms u32[nterms, nparts] = the output term's index in each part (0xffffffff: absent) ->
        (index bytes, term table u32[nterms, 3], stats)."""
        pt = np.ascontiguousarray(part_terms, dtype=np.uint32).reshape(-1, len(parts))
        hs = (C.c_void_p * len(parts))(*[p.h for p in parts])
        terms = np.zeros((max(1, pt.shape[0]), 3), dtype=np.uint32)
        ln = C.c_size_t()
        stats = np.zeros(4, dtype=np.uint64)
        L = hip_lib()
        call = lambda out, cap: L.tri_merge_google(self.h, hs, len(parts), pt.ctypes.data, pt.shape[0], out, cap, C.byref(ln), terms.ctypes.data, stats.ctypes.data)
        (out,) = _size_then_fill(call, [ln])
        return out, terms[: pt.shape[0]], _commit_stats(stats)

    def merge_lucene(self, parts, part_terms):
        """Codecs::Lucene::IndexSession::merge for a whole dictionary (tri_merge_lucene): parts = lucene_codec Index objects uploaded with their hits.data, most recent
        first -> (index bytes, hits.data bytes, term table u32[nterms, 3], stats)."""
        pt = np.ascontiguousarray(part_terms, dtype=np.uint32).reshape(-1, len(parts))
        hs = (C.c_void_p * len(parts))(*[p.h for p in parts])
        terms = np.zeros((max(1, pt.shape[0]), 3), dtype=np.uint32)
        ln, hl = C.c_size_t(), C.c_size_t()
        stats = np.zeros(4, dtype=np.uint64)
        L = hip_lib()
        call = lambda out, cap, hout, hcap: L.tri_merge_lucene(self.h, hs, len(parts), pt.ctypes.data, pt.shape[0], out, cap, C.byref(ln), hout, hcap, C.byref(hl), terms.ctypes.data, stats.ctypes.data)
        out, hout = _size_then_fill(call, [ln, hl])
        return out, hout, terms[: pt.shape[0]], _commit_stats(stats)

    def close(self):
        if self.h:
            hip_lib().tri_dev_close(self.h)
            self.h = C.c_void_p()


class Intersection:
    """The answers of one tri_isect_run call."""

    def __init__(self, h, nreq):
        self.h, self.nreq = h, nreq

    def status(self):
        st = np.zeros(max(1, self.nreq), dtype=np.int32)
        _check(hip_lib().tri_isect_status(self.h, st.ctypes.data))
        return st[: self.nreq].tolist()

    def results(self, r):
        """request r's list as intersect_impl appends it: [(mask, count)] in finalize's order (ties by ascending mask)"""
        n = C.c_size_t()
        _check(hip_lib().tri_isect_results(self.h, r, None, None, 0, C.byref(n)))
        m, c = np.zeros(max(1, n.value), dtype=np.uint64), np.zeros(max(1, n.value), dtype=np.uint32)
        _check(hip_lib().tri_isect_results(self.h, r, m.ctypes.data, c.ctypes.data, n.value, C.byref(n)))
        return list(zip(m[: n.value].tolist(), c[: n.value].tolist()))

    def histogram(self, r):
        """table H of request r: [(mask, documents, first docID)], ascending mask"""
        n = C.c_size_t()
        _check(hip_lib().tri_isect_histogram(self.h, r, None, None, None, 0, C.byref(n)))
        m, c, f = np.zeros(max(1, n.value), dtype=np.uint64), np.zeros(max(1, n.value), dtype=np.uint32), np.zeros(max(1, n.value), dtype=np.uint32)
        _check(hip_lib().tri_isect_histogram(self.h, r, m.ctypes.data, c.ctypes.data, f.ctypes.data, n.value, C.byref(n)))
        return list(zip(m[: n.value].tolist(), c[: n.value].tolist(), f[: n.value].tolist()))

    def info(self):
        i = TriIsectInfo()
        _check(hip_lib().tri_isect_get_info(self.h, C.byref(i)))
        out = {k: getattr(i, k) for k, _ in TriIsectInfo._fields_[:10]}
        for k in ("h_size", "c_size", "lds_spills"):
            out[k] = [getattr(i, k)[r] for r in range(self.nreq)]
        return out

    def close(self):
        if self.h:
            hip_lib().tri_isect_destroy(self.h)
            self.h = C.c_void_p()


def perc_docs(doc_first, terms, freqs, positions, reserved=0):
    """(tri_perc_docs, the arrays it points into) of a batch of documents: doc_first[ndocs + 1] into terms / freqs, positions concatenated."""
    keep = (np.ascontiguousarray(doc_first, dtype=np.uint64), np.ascontiguousarray(terms, dtype=np.uint32), np.ascontiguousarray(freqs, dtype=np.uint32),
            np.ascontiguousarray(positions, dtype=np.uint16))  # fmt: skip
    d = TriPercDocs(keep[0].size - 1, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, keep[3].size, reserved)
    return d, keep


class PercolatorResult:
    """The answer of one tri_perc_match call."""

    def __init__(self, h, ndocs):
        self.h, self.ndocs = h, ndocs

    def pairs(self, order=PERC_BY_QUERY):
        """(queries, documents) of every matching pair, in `order` (PERC_BY_QUERY / PERC_BY_DOCUMENT)."""
        n = C.c_size_t()
        _check(hip_lib().tri_perc_result_pairs(self.h, order, None, None, 0, C.byref(n)))
        q, d = np.zeros(max(1, n.value), dtype=np.uint32), np.zeros(max(1, n.value), dtype=np.uint32)
        _check(hip_lib().tri_perc_result_pairs(self.h, order, q.ctypes.data, d.ctypes.data, n.value, C.byref(n)))
        return q[: n.value], d[: n.value]

    def doc_counts(self):
        c = np.zeros(self.ndocs, dtype=np.uint32)
        _check(hip_lib().tri_perc_result_doc_counts(self.h, c.ctypes.data))
        return c

    @property
    def info(self):
        i = TriPercResultInfo()
        _check(hip_lib().tri_perc_result_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in TriPercResultInfo._fields_ if k != "reserved"}

    def close(self):
        if self.h:
            hip_lib().tri_perc_result_destroy(self.h)
            self.h = None


class Percolator:
    """A resident set of stored queries (tri_perc_create, percolator.h:47-58): postfix programs whose TERM operands index the percolator's own
    dictionary 0 .. nterms-1.  match(documents) tests a batch of documents against all of them."""

    def __init__(self, dev, programs, nterms):
        flat_prog, q = flatten(programs)
        self.dev, self.nq, self.h = dev, len(programs), C.c_void_p()
        _check(hip_lib().tri_perc_create(dev.h, flat_prog.ctypes.data, flat_prog.size, q.ctypes.data, self.nq, nterms, C.byref(self.h)))

    @classmethod
    def create(cls, dev, programs, nterms):
        return cls(dev, programs, nterms)

    @classmethod
    def from_flat(cls, dev, flat_prog, queries, nterms):
        """a set laid out by the caller: the flat u32 program and the (nq, 2) u32 table of (offset, length), as flatten() returns them"""
        self = object.__new__(cls)
        self.dev, self.nq, self.h = dev, len(queries), C.c_void_p()
        _check(hip_lib().tri_perc_create(dev.h, flat_prog.ctypes.data, flat_prog.size, queries.ctypes.data, self.nq, nterms, C.byref(self.h)))
        return self

    def status(self):
        st = np.zeros(max(1, self.nq), dtype=np.int32)
        _check(hip_lib().tri_perc_query_status(self.h, st.ctypes.data))
        return st[: self.nq]

    def set_enabled(self, queries, enabled=True):
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        _check(hip_lib().tri_perc_set_enabled(self.h, q.ctypes.data, q.size, int(bool(enabled))))

    @property
    def info(self):
        i = TriPercInfo()
        _check(hip_lib().tri_perc_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in TriPercInfo._fields_ if k != "reserved"}

    def match(self, doc_first, terms, freqs, positions):
        d, keep = perc_docs(doc_first, terms, freqs, positions)
        r = C.c_void_p()
        _check(hip_lib().tri_perc_match(self.h, C.byref(d), C.byref(r)))
        return PercolatorResult(r, d.ndocs)

    def close(self):
        if self.h:
            hip_lib().tri_perc_destroy(self.h)
            self.h = None


def host_encode_google(docs, freqs, positions, term_first, payload_lens=None, payloads=None):
    """The HOST encoder (csrc/host/google_encoder.hpp: byte-identical to the reference's) over the same arguments: tests' checker of
    Device.encode_google."""
    d = np.ascontiguousarray(docs, dtype=np.uint32)
    f = np.ascontiguousarray(freqs, dtype=np.uint32)
    p = np.ascontiguousarray(positions, dtype=np.uint16)
    tf = np.ascontiguousarray(term_first, dtype=np.uint64)
    pl = None if payload_lens is None else np.ascontiguousarray(payload_lens, dtype=np.uint8)
    pv = None if payload_lens is None else np.ascontiguousarray(payloads, dtype=np.uint64)
    n = tf.size - 1
    terms = np.zeros((max(n, 1), 3), dtype=np.uint32)
    out = np.zeros(int(d.size * 10 + p.size * 13 + 16 * (n + 1) + 64), dtype=np.uint8)
    L = host_lib()
    ln = L.tri_host_encode_google_payloads(d.ctypes.data, f.ctypes.data, p.ctypes.data, None if pl is None else pl.ctypes.data, None if pv is None else pv.ctypes.data,
                                           tf.ctypes.data, n, out.ctypes.data, out.size, terms.ctypes.data)  # fmt: skip
    if ln < 0:
        raise TrinityError("host encoder failed")
    return out[:ln], terms[:n]


class Index:
    def __init__(self, dev, index_bytes, terms, docs_cnt, codec=CODEC_GOOGLE, hits=None):
        self.dev = dev
        b = np.ascontiguousarray(index_bytes, dtype=np.uint8)
        t = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1, 3)
        h = np.ascontiguousarray(hits, dtype=np.uint8) if hits is not None and len(hits) else None
        self.nterms = t.shape[0]
        self.h = C.c_void_p()
        _check(hip_lib().tri_index_upload(dev.h, b.ctypes.data, b.size, h.ctypes.data if h is not None else None, h.size if h is not None else 0, codec, t.ctypes.data, t.shape[0], docs_cnt, C.byref(self.h)))

    @classmethod
    def from_segment(cls, dev, seg):
        return cls(dev, seg.index, seg.terms, seg.docs_cnt, codec=getattr(seg, "codec", CODEC_GOOGLE), hits=getattr(seg, "hits", None))

    def info(self):
        i = TriIndexInfo()
        _check(hip_lib().tri_index_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in TriIndexInfo._fields_}

    def set_masked(self, docids):
        """Replace the segment's masked-document set (masked_documents_registry::test, docidupdates.h:90-119)."""
        d = np.ascontiguousarray(docids, dtype=np.uint32)
        _check(hip_lib().tri_index_set_masked(self.h, d.ctypes.data if d.size else None, d.size))

    def term_docbytes(self, terms):
        t = np.ascontiguousarray(terms, dtype=np.uint32)
        out = np.zeros(t.size, dtype=np.uint64)
        _check(hip_lib().tri_index_term_docbytes(self.h, t.ctypes.data, t.size, out.ctypes.data))
        return out

    def decode_terms(self, terms, df, want_freqs=True):
        """GPU decode of whole postings lists; df = documents per requested term (sizes the host buffers)."""
        t = np.ascontiguousarray(terms, dtype=np.uint32)
        tot = int(np.sum(df))
        docs = np.zeros(tot, dtype=np.uint32)
        freqs = np.zeros(tot, dtype=np.uint32) if want_freqs else None
        offs = np.zeros(t.size + 1, dtype=np.uint64)
        _check(hip_lib().tri_decode_terms(self.h, t.ctypes.data, t.size, docs.ctypes.data, freqs.ctypes.data if want_freqs else None, offs.ctypes.data))
        assert int(offs[-1]) == tot, (int(offs[-1]), tot)
        return docs, freqs, offs

    def intersect(self, requests):
        """Trinity::intersect for a batch of requests (tri_isect_run, intersect.cpp:5-170).  requests: [(groups, stopwords_mask)], groups = lists of term ids
        (0xffffffff: a token the dictionary does not know).  -> Intersection; close() it."""
        reqs = (TriIsectRequest * max(1, len(requests)))()
        terms, first = [], [0]
        for r, (groups, stop) in enumerate(requests):
            reqs[r].ngroups, reqs[r].reserved, reqs[r].stopwords_mask = len(groups), 0, int(stop)
            for g in groups:
                terms += [int(t) for t in g]
                first.append(len(terms))
        t = np.array(terms + [0], dtype=np.uint32)
        gf = np.array(first, dtype=np.uint32)
        h = C.c_void_p()
        _check(hip_lib().tri_isect_run(self.h, reqs, len(requests), t.ctypes.data, gf.ctypes.data, C.byref(h)))
        return Intersection(h, len(requests))

    def decode_hits(self, terms, want_payloads=False):
        """The hits of whole postings lists (tri_decode_hits: materialize_hits for every document, in list order), sized then filled.
        -> (positions u16, payload lengths u8, payload words u64, offsets u64[n + 1] in hits); lengths and words are None unless want_payloads."""
        t = np.ascontiguousarray(terms, dtype=np.uint32)
        offs = np.zeros(t.size + 1, dtype=np.uint64)
        _check(hip_lib().tri_decode_hits(self.h, t.ctypes.data, t.size, None, None, None, 0, offs.ctypes.data))
        tot = int(offs[-1])
        pos = np.zeros(max(1, tot), dtype=np.uint16)
        lens = np.zeros(max(1, tot), dtype=np.uint8) if want_payloads else None
        words = np.zeros(max(1, tot), dtype=np.uint64) if want_payloads else None
        _check(hip_lib().tri_decode_hits(self.h, t.ctypes.data, t.size, pos.ctypes.data, lens.ctypes.data if want_payloads else None, words.ctypes.data if want_payloads else None,
                                         tot, offs.ctypes.data))  # fmt: skip
        assert int(offs[-1]) == tot
        return pos[:tot], lens[:tot] if want_payloads else None, words[:tot] if want_payloads else None, offs

    def decode_hits_at(self, terms, docids, want_payloads=False):
        """The hits of terms[i] in document docids[i] (tri_decode_hits_at), sized then filled.  -> (freqs u32[n]: the stored frequency, 0xffffffff where the
        list does not hold the document; positions, payload lengths, payload words as decode_hits; offsets u64[n + 1])."""
        t = np.ascontiguousarray(terms, dtype=np.uint32)
        d = np.ascontiguousarray(docids, dtype=np.uint32)
        assert t.size == d.size
        freqs = np.zeros(max(1, t.size), dtype=np.uint32)
        offs = np.zeros(t.size + 1, dtype=np.uint64)
        _check(hip_lib().tri_decode_hits_at(self.h, t.ctypes.data, d.ctypes.data, t.size, freqs.ctypes.data, None, None, None, 0, offs.ctypes.data))
        tot = int(offs[-1])
        pos = np.zeros(max(1, tot), dtype=np.uint16)
        lens = np.zeros(max(1, tot), dtype=np.uint8) if want_payloads else None
        words = np.zeros(max(1, tot), dtype=np.uint64) if want_payloads else None
        _check(hip_lib().tri_decode_hits_at(self.h, t.ctypes.data, d.ctypes.data, t.size, freqs.ctypes.data, pos.ctypes.data, lens.ctypes.data if want_payloads else None,
                                            words.ctypes.data if want_payloads else None, tot, offs.ctypes.data))  # fmt: skip
        return freqs[: t.size], pos[:tot], lens[:tot] if want_payloads else None, words[:tot] if want_payloads else None, offs

    def close(self):
        if self.h:
            hip_lib().tri_index_destroy(self.h)
            self.h = C.c_void_p()


FILTER_DROP, FILTER_KEEP = 0, 1
NO_FILTER = 0xFFFFFFFF


class Filter:
    """A per-query document filter on the device (IndexDocumentsFilter, matches.h:190-201): docids = the documents a query that names the
    filter never matches — or, keep=True, the only ones it may match.  Closed before its index; alive while a batch that names it may run."""

    def __init__(self, index, docids, keep=False):
        self.index = index
        d = np.ascontiguousarray(docids, dtype=np.uint32)
        self.h = C.c_void_p()
        _check(hip_lib().tri_filter_create(index.h, d.ctypes.data if d.size else None, d.size, FILTER_KEEP if keep else FILTER_DROP, C.byref(self.h)))

    @classmethod
    def from_docset(cls, batch, q, keep=True):
        """The docID set of query q of a synced DocumentsOnly batch, taken on the device: by default an allow-list (queries restricted to it)."""
        f = cls.__new__(cls)
        f.index = batch.index
        f.h = C.c_void_p()
        _check(hip_lib().tri_filter_from_docset(batch.h, q, FILTER_KEEP if keep else FILTER_DROP, C.byref(f.h)))
        return f

    @classmethod
    def from_columns(cls, index, predicates, keep=True):
        """One filter per Predicate, evaluated on the device over the index's resident columns in one launch (tri_filters_from_columns): by default the documents a
        predicate holds for are the only ones a query may match; keep=False drops them.  All of them, or TrinityError and none."""
        preds = list(predicates)
        raw = (TriPredicate * max(1, len(preds)))()
        alive = []  # the clause arrays and set arrays the structs point into
        for r, p in zip(raw, preds):
            cl = (TriClause * max(1, len(p.clauses)))()
            for c, x in zip(cl, p.clauses):
                c.column, c.kind, c.negate, c.lo, c.hi = x.column.h, x.kind, int(bool(x.negate)), x.lo, x.hi
                if x.values is not None:
                    v = np.ascontiguousarray(x.values, dtype=np.uint32)
                    alive.append(v)
                    c.set, c.nset = (v.ctypes.data if v.size else None), v.size
            alive.append(cl)
            r.clauses, r.nclauses, r.any, r.also = cl, len(p.clauses), int(bool(p.any)), (p.also.h if p.also is not None else None)
        out = (C.c_void_p * max(1, len(preds)))()
        _check(hip_lib().tri_filters_from_columns(index.h, raw, len(preds), FILTER_KEEP if keep else FILTER_DROP, out))
        made = []
        for h in out[: len(preds)]:
            f = cls.__new__(cls)
            f.index, f.h = index, C.c_void_p(h)
            made.append(f)
        return made

    def bitmap(self):
        """The filter's drop bitmap as the kernels read it (tri_filter_bitmap): u32 words, bit d & 31 of word d >> 5 set = document d is dropped.  Bit 0 and the bits
        past the index's largest document are unspecified."""
        n = C.c_size_t()
        probe = np.zeros(1, dtype=np.uint32)
        hip_lib().tri_filter_bitmap(self.h, probe.ctypes.data, 0, C.byref(n))  # (refused for its capacity: leaves the extent)
        words = np.zeros(max(1, n.value), dtype=np.uint32)
        _check(hip_lib().tri_filter_bitmap(self.h, words.ctypes.data, words.size, C.byref(n)))
        return words[: n.value]

    def close(self):
        if self.h:
            hip_lib().tri_filter_destroy(self.h)
            self.h = C.c_void_p()


CLAUSE_RANGE, CLAUSE_SET = 0, 1  # TRI_CLAUSE_RANGE, TRI_CLAUSE_SET
PRED_MAX_CLAUSES, PRED_MAX_COLUMNS, PREDS_MAX = 8, 8, 256  # TRI_PRED_MAX_CLAUSES, TRI_PRED_MAX_COLUMNS, TRI_PREDS_MAX


class Clause:
    """One test of a column predicate (tri_clause).  Clause.range(column, lo, hi): lo <= values[d] <= hi, unsigned, both ends inclusive; Clause.among(column, values):
    values[d] is one of `values` (each below FACET_MAX_BUCKETS).  negate=True: the clause holds where the test fails."""

    def __init__(self, column, kind, lo=0, hi=0, values=None, negate=False):
        self.column, self.kind, self.lo, self.hi, self.values, self.negate = column, kind, lo, hi, values, negate

    @classmethod
    def range(cls, column, lo, hi, negate=False):
        return cls(column, CLAUSE_RANGE, lo=lo, hi=hi, negate=negate)

    @classmethod
    def among(cls, column, values, negate=False):
        return cls(column, CLAUSE_SET, values=np.asarray(values, dtype=np.uint32), negate=negate)


class Predicate:
    """1 .. PRED_MAX_CLAUSES clauses (tri_predicate): it holds for a document when every clause does, or with any=True when at least one does.  also: a Filter of the
    same index whose dropped documents the resulting filter drops too."""

    def __init__(self, clauses, any=False, also=None):
        self.clauses, self.any, self.also = list(clauses), any, also


FACETS_MAX = 4  # TRI_FACETS_MAX
FACET_MAX_BUCKETS = 65536  # TRI_FACET_MAX_BUCKETS
ORDER_MAX_TOPK = 256  # TRI_ORDER_MAX_TOPK


STATS_MAX = 4  # TRI_STATS_MAX
Stats = collections.namedtuple("Stats", "sums counts mins maxs")  # what Batch.stats / CollectionBatch.stats return: one array per plane, [nq, nbuckets + 1]


class Column:
    """A per-document attribute column on the device (tri_column_create): values[d] = the attribute of docID d, docs_cnt + 1 entries (values[0] is never read).
    Closed before its index; alive while a batch that names it may run."""

    def __init__(self, index, values):
        self.index = index
        v = np.ascontiguousarray(values, dtype=np.uint32)
        self.h = C.c_void_p()
        _check(hip_lib().tri_column_create(index.h, v.ctypes.data if v.size else None, v.size, C.byref(self.h)))

    def close(self):
        if self.h:
            hip_lib().tri_column_destroy(self.h)
            self.h = C.c_void_p()


class Batch:
    """A compiled batch of postfix query programs."""

    def __init__(self, index, programs, flags, topk=0, similarity=0, allow_unsupported=False, flat=None):
        """programs: a list of postfix programs (u32 arrays) — or flat = flatten(programs), the (program, tri_query table) pair the C-ABI
        takes, prepared once by a caller that compiles the same queries again and again (bench.py's end-to-end loop).
        A query whose shape the planner does not lower is left out of the batch with a per-query status (it reports no matches): unless
        the caller says it handles that (allow_unsupported=True, then query_status()), such a batch raises instead of answering silently."""
        self.index = index
        self.nq = len(programs) if flat is None else flat[1].shape[0]
        flat, q = flatten(programs) if flat is None else flat
        self.flags, self.topk = flags, topk
        self.h = C.c_void_p()
        _check(hip_lib().tri_batch_create(index.h, flat.ctypes.data, flat.size, q.ctypes.data, self.nq, None, flags, topk, similarity, C.byref(self.h)))
        if not allow_unsupported:
            n = self.info()["unsupported_queries"]
            if n:
                msg = hip_lib().tri_last_error().decode()
                self.close()
                raise TrinityError(f"{n} queries of the batch have a shape the planner does not lower (allow_unsupported=True + query_status() to run the rest): {msg}")

    @classmethod
    def conjunctions(cls, index, term_rows, flags=FLAG_DOCUMENTS_ONLY, topk=0):
        rows = np.asarray(term_rows, dtype=np.uint32)
        k = rows.shape[1]
        progs = np.empty((rows.shape[0], k + 1), dtype=np.uint32)
        progs[:, :k] = rows  # TERM tokens: op 0 => the raw term id
        progs[:, k] = tok(OP_AND, k)
        return cls(index, list(progs), flags, topk)

    def query_status(self):
        """Per query: 0, or the status (TRI_ERR_UNSUPPORTED = -3) with which the planner left it out of the batch."""
        out = np.zeros(self.nq, dtype=np.int32)
        _check(hip_lib().tri_batch_query_status(self.h, out.ctypes.data))
        return out

    def set_filters(self, filters, filter_of_query=None):
        """Per-query document filters for the runs that follow (tri_batch_set_filters): filter_of_query[q] = index into `filters` of query q's
        filter, NO_FILTER for none; an empty `filters` clears.  The batch keeps the Filter objects referenced."""
        filters = list(filters)
        foq = np.ascontiguousarray(filter_of_query if filters else [], dtype=np.uint32)
        if filters and foq.size != self.nq:
            raise TrinityError(f"filter_of_query has {foq.size} entries for {self.nq} queries")
        arr = (C.c_void_p * max(1, len(filters)))(*[f.h for f in filters])
        _check(hip_lib().tri_batch_set_filters(self.h, arr if filters else None, len(filters), foq.ctypes.data if filters else None))
        self._filters = filters

    def set_facets(self, facets):
        """Facet counts for the runs that follow (tri_batch_set_facets): facets = [(Column, nbuckets), ...], at most FACETS_MAX; an empty list clears.  Every run then
        counts each query's docID set by the columns' values on the device; results: facets(k).  The batch keeps the Column objects referenced."""
        facets = list(facets)
        arr = (TriFacet * max(1, len(facets)))()
        for i, (col, nb) in enumerate(facets):
            arr[i].column, arr[i].nbuckets, arr[i].reserved = (col.h if col is not None else None), int(nb), 0
        _check(hip_lib().tri_batch_set_facets(self.h, arr if facets else None, len(facets)))
        self._facets = facets

    def facets(self, k):
        """After sync(): facet k's rows, u32[nq, nbuckets + 1] in caller query order — row[q, v] = the documents of query q's docID set whose value is v; the last
        counter takes every value >= nbuckets, so a row sums to counts()[q] (tri_batch_facets: one copy for the whole batch)."""
        spec = getattr(self, "_facets", [])
        nb = int(spec[k][1]) if 0 <= k < len(spec) else 0  # (out of range: the library refuses)
        out = np.zeros((self.nq, nb + 1), dtype=np.uint32)
        _check(hip_lib().tri_batch_facets(self.h, k, out.ctypes.data, out.size))
        return out

    def set_order(self, column, topk, descending=False):
        """Order by a column for the runs that follow (tri_batch_set_order): every run then selects, on the device, each query's first topk documents by
        (column value, docID) — descending: highest value first, ties still to the lower docID; results: ordered().  The batch keeps the Column referenced."""
        spec = TriOrder(column.h if column is not None else None, int(topk), 1 if descending else 0, 0)
        _check(hip_lib().tri_batch_set_order(self.h, C.byref(spec)))
        self._order = (column, int(topk), bool(descending))

    def clear_order(self):
        """Remove the order (tri_batch_set_order with NULL): later runs launch what they did before one was set."""
        _check(hip_lib().tri_batch_set_order(self.h, None))
        self._order = None

    def ordered(self):
        """After sync(): (docids u32[nq, topk], values u32[nq, topk], counts u32[nq]) in caller query order — row q holds the first counts[q] = min(matches, topk)
        documents of query q's docID set by (value, docID), values[q, i] the column's value of docids[q, i]; entries past counts[q] are zero (tri_batch_ordered)."""
        spec = getattr(self, "_order", None)
        k = spec[1] if spec else 1  # (no order: the library refuses)
        d, v, c = np.zeros((self.nq, k), dtype=np.uint32), np.zeros((self.nq, k), dtype=np.uint32), np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_batch_ordered(self.h, d.ctypes.data, v.ctypes.data, c.ctypes.data))
        return d, v, c

    def set_stats(self, stats):
        """Stats of a column for the runs that follow (tri_batch_set_stats): stats = [(group Column or None, nbuckets, value Column), ...], at most STATS_MAX; an empty
        list clears.  nbuckets is 0 without a group column.  Every run then aggregates each query's docID set on the device; results: stats(k).  The batch keeps the
        Column objects referenced."""
        stats = list(stats)
        arr = (TriStat * max(1, len(stats)))()
        for i, (group, nb, value) in enumerate(stats):
            arr[i].group, arr[i].value = (group.h if group is not None else None), (value.h if value is not None else None)
            arr[i].nbuckets, arr[i].reserved = int(nb), 0
        _check(hip_lib().tri_batch_set_stats(self.h, arr if stats else None, len(stats)))
        self._stats = stats

    def stats(self, k):
        """After sync(): stat k's rows as Stats(sums u64, counts u32, mins u32, maxs u32), each [nq, nbuckets + 1] in caller query order — the record of bucket
        min(group[d], nbuckets) over the documents d of query q's docID set; the last is the overflow bucket; an empty record reads 0, 0, 0xffffffff, 0
        (tri_batch_stats: one copy per plane for the whole batch)."""
        spec = getattr(self, "_stats", [])
        nb = int(spec[k][1]) if 0 <= k < len(spec) else 0  # (out of range: the library refuses)
        out = Stats(np.zeros((self.nq, nb + 1), np.uint64), np.zeros((self.nq, nb + 1), np.uint32), np.zeros((self.nq, nb + 1), np.uint32), np.zeros((self.nq, nb + 1), np.uint32))
        _check(hip_lib().tri_batch_stats(self.h, k, out.sums.ctypes.data, out.counts.ctypes.data, out.mins.ctypes.data, out.maxs.ctypes.data, out.sums.size))
        return out

    def set_ranker(self, topk, freq_cap=65535, adjacency=0.0, weights=None):
        """FLAG_MATCHED_TERMS batches: rank every query's matches on the device for the runs that follow (tri_batch_set_ranker, TRI_RANK_PROXIMITY):
        score = sum over the present reportable terms of weight * min(freq, freq_cap), + adjacency per hit of term k that term k + 1 follows at the next
        position.  weights: one per token of the flattened program (as tri_batch_create's), None: 1.0 each.  Results: ranked()."""
        spec = TriRanker(RANK_PROXIMITY, topk, freq_cap, 0, adjacency)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        _check(hip_lib().tri_batch_set_ranker(self.h, C.byref(spec), None if w is None else w.ctypes.data))
        self.rank_topk = topk

    def clear_ranker(self):
        _check(hip_lib().tri_batch_set_ranker(self.h, None, None))
        self.rank_topk = 0

    def ranked(self):
        """After sync(): (docids u32[nq, topk], scores f64[nq, topk], counts u32[nq]) — per query its best min(matches, topk) documents, score descending,
        docID ascending; rows past counts[q] are zero."""
        k = max(1, getattr(self, "rank_topk", 0))
        d = np.zeros((self.nq, k), dtype=np.uint32)
        s = np.zeros((self.nq, k), dtype=np.float64)
        c = np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_batch_ranked(self.h, d.ctypes.data, s.ctypes.data, c.ctypes.data))
        return d, s, c

    def run(self):
        _check(hip_lib().tri_batch_run(self.h))

    def sync(self):
        _check(hip_lib().tri_batch_sync(self.h))

    def info(self):
        i = TriBatchInfo()
        _check(hip_lib().tri_batch_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in TriBatchInfo._fields_}

    def matched_terms(self, q, n):
        """FLAG_MATCHED_TERMS batches: (terms u32[nt], present u32[n], freq u16[n, nt], positions u16[npos]) for the n matches of
        query q (ascending docID, as docset(q, n) returns them); positions are match-major then term-minor.  A wide-report query (17 .. 64 reportable
        terms, option rich_max_terms) goes through the _wide calls: the same shape, present as u64[n]."""
        L = hip_lib()
        terms = np.zeros(64, dtype=np.uint32)
        nt = C.c_uint32()
        _check(L.tri_batch_query_terms_wide(self.h, q, terms.ctypes.data, C.byref(nt)))
        nt = nt.value
        wide = nt > 16
        matched = L.tri_batch_matched_terms_wide if wide else L.tri_batch_matched_terms
        npos = C.c_size_t()
        _check(matched(self.h, q, None, None, None, 0, C.byref(npos)))
        present = np.zeros(n, dtype=np.uint64 if wide else np.uint32)
        freq = np.zeros((n, max(nt, 1)), dtype=np.uint16)
        pos = np.zeros(max(1, npos.value), dtype=np.uint16)
        _check(matched(self.h, q, present.ctypes.data, freq.ctypes.data, pos.ctypes.data, pos.size, C.byref(npos)))
        return terms[:nt], present, freq[:, :nt], pos[: npos.value]

    def matched_terms_wide(self, q, n):
        """... through the _wide calls whatever the query's width: present as u64[n] (a query of at most 16 terms: zero-extended)."""
        L = hip_lib()
        terms = np.zeros(64, dtype=np.uint32)
        nt = C.c_uint32()
        _check(L.tri_batch_query_terms_wide(self.h, q, terms.ctypes.data, C.byref(nt)))
        nt = nt.value
        npos = C.c_size_t()
        _check(L.tri_batch_matched_terms_wide(self.h, q, None, None, None, 0, C.byref(npos)))
        present = np.zeros(n, dtype=np.uint64)
        freq = np.zeros((n, max(nt, 1)), dtype=np.uint16)
        pos = np.zeros(max(1, npos.value), dtype=np.uint16)
        _check(L.tri_batch_matched_terms_wide(self.h, q, present.ctypes.data, freq.ctypes.data, pos.ctypes.data, pos.size, C.byref(npos)))
        return terms[:nt], present, freq[:, :nt], pos[: npos.value]

    def counts(self):
        out = np.zeros(self.nq, dtype=np.uint64)
        _check(hip_lib().tri_batch_match_counts(self.h, out.ctypes.data))
        return out

    def docset(self, q, n=None):
        if n is None:
            n = int(self.counts()[q])
        out = np.zeros(n, dtype=np.uint32)
        got = C.c_size_t()
        _check(hip_lib().tri_batch_docset(self.h, q, out.ctypes.data, n, C.byref(got)))
        return out[: got.value]

    def docsets(self, out=None):
        """Every query's docID set in one call (tri_batch_docsets): (flat u32[], offsets u64[nq + 1]) — query q's ascending docIDs are
        flat[offsets[q]:offsets[q + 1]].  `out`: a caller's u32 buffer (numpy array or anything with ctypes.data / data_ptr(): pinned memory makes
        the one device-to-host copy run at PCIe's rate); None: a fresh array of the exact size."""
        L = hip_lib()
        offs = np.zeros(self.nq + 1, dtype=np.uint64)
        _check(L.tri_batch_docsets(self.h, None, 0, offs.ctypes.data))
        total = int(offs[-1])
        if out is None:
            out = np.zeros(max(1, total), dtype=np.uint32)
        ptr, cap = (out.data_ptr(), out.numel()) if hasattr(out, "data_ptr") else (out.ctypes.data, out.size)
        _check(L.tri_batch_docsets(self.h, ptr, cap, offs.ctypes.data))
        return out, offs

    def docsets_mixed(self, out=None):
        """Every query's docID set in the form the engine holds it (tri_batch_docsets_mixed): (flat u32[], offsets u64[nq + 1], forms u32[nq]) — forms[q] = 0:
        flat[offsets[q]:offsets[q + 1]] = query q's ascending docIDs; 1: the words of a bitmap over its docID range (bit j of word i = document 32 i + j)."""
        L = hip_lib()
        offs = np.zeros(self.nq + 1, dtype=np.uint64)
        forms = np.zeros(max(1, self.nq), dtype=np.uint32)
        _check(L.tri_batch_docsets_mixed(self.h, None, 0, offs.ctypes.data, forms.ctypes.data))
        total = int(offs[-1])
        if out is None:
            out = np.zeros(max(1, total), dtype=np.uint32)
        ptr, cap = (out.data_ptr(), out.numel()) if hasattr(out, "data_ptr") else (out.ctypes.data, out.size)
        _check(L.tri_batch_docsets_mixed(self.h, ptr, cap, offs.ctypes.data, forms.ctypes.data))
        return out, offs, forms[: self.nq]

    def docset_form(self, q):
        """1 when the engine holds query q's docID set as a bitmap (RESULT_BITMAP), 0: ascending docIDs."""
        form, first, nw = C.c_int(), C.c_uint32(), C.c_size_t()
        _check(hip_lib().tri_batch_docset_bitmap(self.h, q, C.byref(form), None, 0, C.byref(first), C.byref(nw)))
        return form.value

    def docset_bitmap_words(self, q):
        """Words of query q's result bitmap (0: its docID set is held as ascending docIDs)."""
        form, first, nw = C.c_int(), C.c_uint32(), C.c_size_t()
        _check(hip_lib().tri_batch_docset_bitmap(self.h, q, C.byref(form), None, 0, C.byref(first), C.byref(nw)))
        return int(nw.value) if form.value else 0

    def docset_bitmap(self, q):
        """None when the engine holds query q's docID set as ascending docIDs; else (first_doc, words u32[]): bit j of words[i] = document
        first_doc + 32 i + j matches (DocumentsOnly queries expected to match one document in 32 or more; option result_bitmaps)."""
        L = hip_lib()
        form, first, nw = C.c_int(), C.c_uint32(), C.c_size_t()
        _check(L.tri_batch_docset_bitmap(self.h, q, C.byref(form), None, 0, C.byref(first), C.byref(nw)))
        if not form.value:
            return None
        words = np.zeros(nw.value, dtype=np.uint32)
        _check(L.tri_batch_docset_bitmap(self.h, q, C.byref(form), words.ctypes.data, nw.value, C.byref(first), C.byref(nw)))
        return first.value, words

    def matched_payloads(self, q):
        """FLAG_MATCHED_TERMS | FLAG_HIT_PAYLOADS batches: (lens u8[npos], payloads u64[npos]) parallel to matched_terms()'s positions."""
        L = hip_lib()
        n = C.c_size_t()
        _check(L.tri_batch_matched_payloads(self.h, q, None, None, 0, C.byref(n)))
        lens = np.zeros(max(1, n.value), dtype=np.uint8)
        pl = np.zeros(max(1, n.value), dtype=np.uint64)
        _check(L.tri_batch_matched_payloads(self.h, q, lens.ctypes.data, pl.ctypes.data, n.value, C.byref(n)))
        return lens[: n.value], pl[: n.value]

    def scores(self, q, n=None):
        if n is None:
            n = int(self.counts()[q])
        out = np.zeros(n, dtype=np.float64)
        got = C.c_size_t()
        _check(hip_lib().tri_batch_scores(self.h, q, out.ctypes.data, n, C.byref(got)))
        return out[: got.value]

    def docset_hashes(self):
        out = np.zeros(self.nq, dtype=np.uint64)
        _check(hip_lib().tri_batch_docset_hashes(self.h, out.ctypes.data))
        return out

    def device_results(self):
        """Raw device pointers of the result blocks the multi-GPU gather sends: {"counts": u64[nq]} and, for AccumulatedScore top-K
        batches, {"docs": u32[nq][k], "scores": f32[nq][k], "topk_counts": u32[nq]}.  Valid after the run completed on the engine stream."""
        L = hip_lib()
        p = C.c_void_p()
        _check(L.tri_batch_counts_device(self.h, C.byref(p)))
        out = {"counts": p.value}
        if (self.flags & FLAG_ACCUMULATED_SCORE) and self.topk:
            d, s, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
            _check(L.tri_batch_topk_device(self.h, C.byref(d), C.byref(s), C.byref(c)))
            out.update(docs=d.value, scores=s.value, topk_counts=c.value)
        return out

    def topk_results(self):
        d = np.zeros((self.nq, self.topk), dtype=np.uint32)
        s = np.zeros((self.nq, self.topk), dtype=np.float32)
        c = np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_batch_topk(self.h, d.ctypes.data, s.ctypes.data, c.ctypes.data))
        return d, s, c

    def close(self):
        if self.h:
            hip_lib().tri_batch_destroy(self.h)
            self.h = C.c_void_p()

class CollectionBatch:
    """The same queries over the sources of a collection (IndexSourcesCollection): one Batch per source, oldest first, each index
    carrying the documents the newer sources update as its masked set; counts add up, top-K lists merge on the device."""

    def __init__(self, batches, allow_unsupported=False):
        self.parts = list(batches)
        self.nq, self.topk = self.parts[0].nq, self.parts[0].topk
        arr = (C.c_void_p * len(self.parts))(*[b.h for b in self.parts])
        self.h = C.c_void_p()
        _check(hip_lib().tri_cbatch_create(arr, len(self.parts), C.byref(self.h)))
        if not allow_unsupported and self.query_status().any():
            self.close()
            raise TrinityError("queries of the collection batch have a shape the planner does not lower (allow_unsupported=True + query_status())")

    def query_status(self):
        out = np.zeros(self.nq, dtype=np.int32)
        _check(hip_lib().tri_cbatch_query_status(self.h, out.ctypes.data))
        return out

    def run(self):
        _check(hip_lib().tri_cbatch_run(self.h))

    def sync(self):
        _check(hip_lib().tri_cbatch_sync(self.h))

    def counts(self):
        out = np.zeros(self.nq, dtype=np.uint64)
        _check(hip_lib().tri_cbatch_match_counts(self.h, out.ctypes.data))
        return out

    def topk_results(self):
        d = np.zeros((self.nq, self.topk), dtype=np.uint32)
        s = np.zeros((self.nq, self.topk), dtype=np.float32)
        c = np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_cbatch_topk(self.h, d.ctypes.data, s.ctypes.data, c.ctypes.data))
        return d, s, c

    def docset(self, q, n):
        out = np.zeros(max(1, n), dtype=np.uint32)
        got = C.c_size_t()
        _check(hip_lib().tri_cbatch_docset(self.h, q, out.ctypes.data, n, C.byref(got)))
        return out[: got.value]

    def ranked(self):
        """After sync(), every part carrying the same ranker (Batch.set_ranker): (docids u32[nq, topk], scores f64[nq, topk], counts u32[nq]) — per query the
        best topk documents over all parts, score descending, docID ascending, older source first; rows past counts[q] are zero (tri_cbatch_ranked)."""
        k = max(1, max(getattr(b, "rank_topk", 0) for b in self.parts))
        d = np.zeros((self.nq, k), dtype=np.uint32)
        s = np.zeros((self.nq, k), dtype=np.float64)
        c = np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_cbatch_ranked(self.h, d.ctypes.data, s.ctypes.data, c.ctypes.data))
        return d, s, c

    def facets(self, k):
        """After sync(): facet k's rows over the collection, u64[nq, nbuckets + 1] — the parts' rows summed (tri_cbatch_facets); the parts must agree in the number
        of facets and in facet k's nbuckets."""
        spec = getattr(self.parts[0], "_facets", [])
        nb = int(spec[k][1]) if 0 <= k < len(spec) else 0
        out = np.zeros((self.nq, nb + 1), dtype=np.uint64)
        _check(hip_lib().tri_cbatch_facets(self.h, k, out.ctypes.data, out.size))
        return out

    def ordered(self):
        """After sync(): (docids, values, counts) over the collection — the parts' ordered lists merged per query by (value, docID, source), cut at topk
        (tri_cbatch_ordered); every part must carry an order of the same topk and direction."""
        ks = [getattr(p, "_order", None) for p in self.parts]
        k = max([o[1] for o in ks if o] or [1])  # (parts that disagree, or none ordered: the library refuses)
        d, v, c = np.zeros((self.nq, k), dtype=np.uint32), np.zeros((self.nq, k), dtype=np.uint32), np.zeros(self.nq, dtype=np.uint32)
        _check(hip_lib().tri_cbatch_ordered(self.h, d.ctypes.data, v.ctypes.data, c.ctypes.data))
        return d, v, c

    def stats(self, k):
        """After sync(): stat k's rows over the collection as Stats(sums u64, counts u64, mins u32, maxs u32), each [nq, nbuckets + 1] — the parts' rows combined
        (tri_cbatch_stats); the parts must agree in the number of stats, in stat k's nbuckets and in whether it is grouped."""
        spec = getattr(self.parts[0], "_stats", [])
        nb = int(spec[k][1]) if 0 <= k < len(spec) else 0
        out = Stats(np.zeros((self.nq, nb + 1), np.uint64), np.zeros((self.nq, nb + 1), np.uint64), np.zeros((self.nq, nb + 1), np.uint32), np.zeros((self.nq, nb + 1), np.uint32))
        _check(hip_lib().tri_cbatch_stats(self.h, k, out.sums.ctypes.data, out.counts.ctypes.data, out.mins.ctypes.data, out.maxs.ctypes.data, out.sums.size))
        return out

    def _query_width(self, q):
        """(terms, nterms) of query q: those of the first part that reports it (the parts agree, or the row calls refuse)."""
        terms = np.zeros(64, dtype=np.uint32)
        for b in self.parts:
            nt = C.c_uint32()
            _check(hip_lib().tri_batch_query_terms_wide(b.h, q, terms.ctypes.data, C.byref(nt)))
            if nt.value:
                return terms, nt.value
        return terms, 0

    def _matched(self, q, n, wide):
        L = hip_lib()
        matched = L.tri_cbatch_matched_terms_wide if wide else L.tri_cbatch_matched_terms
        terms, nt = self._query_width(q)
        npos = C.c_size_t()
        _check(matched(self.h, q, None, None, None, 0, C.byref(npos)))
        present = np.zeros(n, dtype=np.uint64 if wide else np.uint32)
        freq = np.zeros((n, max(nt, 1)), dtype=np.uint16)
        pos = np.zeros(max(1, npos.value), dtype=np.uint16)
        _check(matched(self.h, q, present.ctypes.data, freq.ctypes.data, pos.ctypes.data, pos.size, C.byref(npos)))
        return terms[:nt], present, freq[:, :nt], pos[: npos.value]

    def matched_terms(self, q, n):
        """FLAG_MATCHED_TERMS parts: what Batch.matched_terms returns, for the n matches docset(q, n) returns — the parts' rows source after source; the terms
        are the first reporting part's (the parts' term ids are their own)."""
        return self._matched(q, n, self._query_width(q)[1] > 16)

    def matched_terms_wide(self, q, n):
        """... through the _wide call whatever the query's width: present as u64[n]."""
        return self._matched(q, n, True)

    def matched_payloads(self, q):
        """FLAG_MATCHED_TERMS | FLAG_HIT_PAYLOADS parts: (lens u8[npos], payloads u64[npos]) parallel to matched_terms()'s positions."""
        L = hip_lib()
        n = C.c_size_t()
        _check(L.tri_cbatch_matched_payloads(self.h, q, None, None, 0, C.byref(n)))
        lens = np.zeros(max(1, n.value), dtype=np.uint8)
        pl = np.zeros(max(1, n.value), dtype=np.uint64)
        _check(L.tri_cbatch_matched_payloads(self.h, q, lens.ctypes.data, pl.ctypes.data, n.value, C.byref(n)))
        return lens[: n.value], pl[: n.value]

    def close(self):
        if self.h:
            hip_lib().tri_cbatch_destroy(self.h)
            self.h = C.c_void_p()
