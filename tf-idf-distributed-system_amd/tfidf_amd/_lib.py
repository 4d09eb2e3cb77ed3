"""ctypes binding of libtfidf.so (include/tfidf.h).

The library is built in-tree (``make -C tf-idf-distributed-system_amd``) and
loaded from ``tf-idf-distributed-system_amd/lib/libtfidf.so``.  There is no
fallback: if the HIP library is missing, every engine call raises.
"""
import ctypes as C
import os
import subprocess

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libtfidf.so")

OK = 0
E_INVALID_ARG = 1
E_HIP = 2
E_OOM = 3
E_UNSUPPORTED_INPUT = 4
E_UNSUPPORTED_QUERY = 5
E_CAPACITY = 6
E_STATE = 7
E_BUFFER = 8
E_NO_DEVICE = 9
E_QUERY_SYNTAX = 10

STATS_SHARD = 0
STATS_GLOBAL = 1

OWN_STREAM = C.c_void_p(-1 & ((1 << 64) - 1))   # TFIDF_OWN_STREAM

INVERSION_AUTO = 0
INVERSION_BLOCK = 1
INVERSION_TERM = 2


class Config(C.Structure):
    _fields_ = [("k1", C.c_float), ("b", C.c_float), ("stats_mode", C.c_int32), ("device", C.c_int32),
                ("vocab_capacity_log2", C.c_uint32), ("max_token_len", C.c_uint32), ("inversion", C.c_int32)]


class IndexStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("num_docs", "doc_count", "sum_ttf", "num_terms", "nnz",
                                          "device_bytes", "long_docs", "text_bytes", "term_major",
                                          "pack_docs", "pack_retried", "unicode_docs", "long_chunked",
                                          "malformed_docs", "hash_seed", "hash_rebuilds",
                                          "coalesced_batches", "coalesced_queries", "unit_batches", "unit_count", "fused_queries",
                                          "unicode_wave_docs", "dead_docs", "dead_bytes", "compactions")]


class CommitTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_total", "ms_tokenize", "ms_long", "ms_df", "ms_blockscan",
                                         "ms_colscan", "ms_scatter")] + \
               [(n, C.c_uint64) for n in ("text_bytes", "num_docs", "nnz")]


class HostProfile(C.Structure):
    """tfidf_host_profile: the host side of the last commit."""
    _fields_ = [(n, C.c_double) for n in ("ms_wall", "ms_counters", "ms_enqueued", "ms_synced", "ms_published")] + \
               [(n, C.c_uint32) for n in ("stream_syncs", "col_rank_runs", "mirror_dict", "mirror_df", "mirror_crank",
                                          "dict_delta_entries", "df_delta_entries")] + \
               [(n, C.c_uint64) for n in ("bytes_dict", "bytes_df", "bytes_crank")]


MIRROR_FORMS = ("none", "delta", "whole")        # TFIDF_MIRROR_*


class TfidfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libtfidf error %d: %s" % (code, msg))
        self.code = code


class UnsupportedQuery(TfidfError):
    pass


class UnsupportedInput(TfidfError):
    pass


class QuerySyntaxError(TfidfError):
    """QueryParser ParseException / TooManyClauses: Worker.processDocuments answers []."""


VP = C.c_void_p
U8P = C.POINTER(C.c_uint8)
U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)
F32P = C.POINTER(C.c_float)
F64P = C.POINTER(C.c_double)


def _fuzzy_batch_sig(df):
    """tfidf_[reader_|node_]fuzzy_terms_batch; df is u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U64P, U64P, U64P, VP,
                      C.c_uint64, df, U8P, C.c_uint64, U64P, U64P, F32P])


_FUZZY_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, U64P, U64P, VP,
                               C.c_uint64, U32P, U8P, C.c_uint64, U64P, U64P, F32P])


# tfidf_[reader_]fuzzy_expand[_batch]: the lookup's layout with the float boosts after dist
_FUZZY_EXPAND_BATCH_SIG = (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U64P, U64P,
                                     U64P, VP, C.c_uint64, U32P, U8P, F32P, C.c_uint64, U64P, U64P, F32P])
_FUZZY_EXPAND_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, U64P, U64P, VP,
                                      C.c_uint64, U32P, U8P, F32P, C.c_uint64, U64P, U64P, F32P])


def _fuzzy_search_batch_sig(doc):
    """tfidf_[reader_|node_]search_fuzzy_batch; doc ids are u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, doc, F32P, C.c_uint64,
                      U64P, U32P, U64P, F32P])


_FUZZY_SEARCH_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, U32P, F32P,
                                      C.c_uint64, U32P, U64P, F32P])


def _wildcard_terms_sig(df):
    """tfidf_[reader_|node_]wildcard_terms_batch; df is u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, U64P, U64P, U64P, VP, C.c_uint64, df, C.c_uint64,
                      U64P, U64P, F32P])


def _wildcard_docs_sig(doc):
    """tfidf_[reader_|node_]search_wildcard_batch; doc ids are u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, doc, C.c_uint64, U64P, U64P, U64P, F32P])


_WILDCARD_TERMS_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U64P, U64P, VP, C.c_uint64, U32P,
                                        C.c_uint64, U64P, U64P, F32P])
_WILDCARD_DOCS_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, C.c_uint64, U64P, U64P, F32P])


class MltParams(C.Structure):
    _fields_ = [("min_tf", C.c_uint32), ("min_df", C.c_uint32), ("max_df", C.c_uint32), ("max_terms", C.c_uint32)]


MLT_EXCLUDE_SEED = 1
MLTP = C.POINTER(MltParams)
# tfidf_[reader_]mlt_terms_batch / tfidf_[reader_]more_like_this_batch / the single forms
_MLT_TERMS_SIG = (C.c_int, [VP, U32P, C.c_uint32, MLTP, U64P, U64P, U64P, VP, C.c_uint64, U32P, U32P, F32P, C.c_uint64,
                            U64P, U64P])
_MLT_BATCH_SIG = (C.c_int, [VP, U32P, C.c_uint32, MLTP, C.c_uint32, C.c_uint32, U32P, F32P, U32P])
_MLT_SINGLE_SIG = (C.c_int, [VP, C.c_uint32, MLTP, C.c_uint32, C.c_uint32, U32P, F32P, U32P])

OCCUR_SHOULD, OCCUR_MUST, OCCUR_MUST_NOT, OCCUR_FILTER = 0, 1, 2, 3                       # TFIDF_OCCUR_*
CLAUSE_TEXT, CLAUSE_PHRASE, CLAUSE_WILDCARD, CLAUSE_REGEX, CLAUSE_FUZZY = 0, 1, 2, 3, 4   # TFIDF_CLAUSE_*


class Clause(C.Structure):
    """tfidf_clause (12 bytes)."""
    _fields_ = [("occur", C.c_uint8), ("kind", C.c_uint8), ("max_edits", C.c_uint8), ("max_expansions", C.c_uint8),
                ("prefix_len", C.c_uint32), ("slop", C.c_uint32)]


CLAUSEP = C.POINTER(Clause)


def _compound_batch_sig(doc):
    """tfidf_[reader_|node_]search_compound_batch; doc ids are u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, CLAUSEP, U64P, C.c_uint32, doc, F32P, C.c_uint64, U64P, U64P, F32P])


_COMPOUND_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, U64P, CLAUSEP, C.c_uint32, U32P, F32P, C.c_uint64, U64P, F32P])

CLAUSE_GROUP = 5                 # TFIDF_CLAUSE_GROUP: nested calls only
QNODE_ROOT = 0xFFFFFFFF          # TFIDF_QNODE_ROOT


class QNode(C.Structure):
    """tfidf_qnode (20 bytes)."""
    _fields_ = Clause._fields_ + [("parent", C.c_uint32), ("min_should_match", C.c_uint32)]


QNODEP = C.POINTER(QNode)


def _nested_batch_sig(doc):
    """tfidf_[reader_|node_]search_nested_batch; doc ids are u32 per shard, u64 over a node."""
    return (C.c_int, [VP, C.c_char_p, U64P, QNODEP, U64P, C.c_uint32, doc, F32P, C.c_uint64, U64P, U64P, F32P])


_NESTED_SINGLE_SIG = (C.c_int, [VP, C.c_char_p, U64P, QNODEP, C.c_uint32, U32P, F32P, C.c_uint64, U64P, F32P])

SIGNATURES = {
    "tfidf_version": (C.c_char_p, []),
    "tfidf_last_error": (C.c_char_p, []),
    "tfidf_config_init": (C.c_int, [C.POINTER(Config)]),
    "tfidf_create": (C.c_int, [C.POINTER(Config), C.POINTER(VP)]),
    "tfidf_destroy": (C.c_int, [VP]),
    "tfidf_add_docs": (C.c_int, [VP, VP, U64P, C.c_uint64, C.c_char_p, U64P]),
    "tfidf_clear": (C.c_int, [VP]),
    "tfidf_save": (C.c_int, [VP, C.c_char_p]),
    "tfidf_load": (C.c_int, [VP, C.c_char_p]),
    "tfidf_add_docs_device": (C.c_int, [VP, VP, VP, C.c_uint64, C.c_uint64]),
    "tfidf_commit": (C.c_int, [VP]),
    "tfidf_delete_docs": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint64, U64P]),
    "tfidf_compact": (C.c_int, [VP, U64P, F32P]),
    "tfidf_set_compact_threshold": (C.c_int, [VP, C.c_uint32]),
    "tfidf_doc_text": (C.c_int, [VP, C.c_uint64, VP, C.c_uint64, U64P]),
    "tfidf_reader_doc_text": (C.c_int, [VP, C.c_uint64, VP, C.c_uint64, U64P]),
    "tfidf_reader_matches": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, C.c_uint64, U64P, U32P, U32P, C.c_uint64,
                                       U64P, U64P, F32P]),
    "tfidf_matches": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, C.c_uint64, U64P, U32P, U32P, C.c_uint64, U64P,
                                U64P, F32P]),
    "tfidf_reader_snippets": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, C.c_uint64, C.c_uint32, VP, C.c_uint64,
                                        U64P, U64P, U64P, U32P, U32P, C.c_uint64, U64P, U64P, U64P, F32P]),
    "tfidf_snippets": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, C.c_uint64, C.c_uint32, VP, C.c_uint64, U64P,
                                 U64P, U64P, U32P, U32P, C.c_uint64, U64P, U64P, U64P, F32P]),
    "tfidf_reader_matches_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, U64P, U64P, U32P, U32P,
                                             C.c_uint64, U64P, U64P, F32P]),
    "tfidf_matches_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, U64P, U64P, U32P, U32P, C.c_uint64,
                                      U64P, U64P, F32P]),
    "tfidf_reader_snippets_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, U64P, C.c_uint32, VP,
                                              C.c_uint64, U64P, U64P, U64P, U32P, U32P, C.c_uint64, U64P, U64P,
                                              U64P, F32P]),
    "tfidf_snippets_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, U64P, C.c_uint32, VP, C.c_uint64,
                                       U64P, U64P, U64P, U32P, U32P, C.c_uint64, U64P, U64P, U64P, F32P]),
    "tfidf_last_highlight_chunks": (C.c_int, [VP, U64P, U64P]),
    "tfidf_fuzzy_terms_batch": _fuzzy_batch_sig(U32P),
    "tfidf_reader_fuzzy_terms_batch": _fuzzy_batch_sig(U32P),
    "tfidf_fuzzy_terms": _FUZZY_SINGLE_SIG,
    "tfidf_reader_fuzzy_terms": _FUZZY_SINGLE_SIG,
    "tfidf_last_fuzzy_chunks": (C.c_int, [VP, U64P, U64P]),
    "tfidf_fuzzy_expand_batch": _FUZZY_EXPAND_BATCH_SIG,
    "tfidf_reader_fuzzy_expand_batch": _FUZZY_EXPAND_BATCH_SIG,
    "tfidf_fuzzy_expand": _FUZZY_EXPAND_SINGLE_SIG,
    "tfidf_reader_fuzzy_expand": _FUZZY_EXPAND_SINGLE_SIG,
    "tfidf_search_fuzzy_batch": _fuzzy_search_batch_sig(U32P),
    "tfidf_reader_search_fuzzy_batch": _fuzzy_search_batch_sig(U32P),
    "tfidf_node_search_fuzzy_batch": _fuzzy_search_batch_sig(U64P),
    "tfidf_search_fuzzy": _FUZZY_SEARCH_SINGLE_SIG,
    "tfidf_reader_search_fuzzy": _FUZZY_SEARCH_SINGLE_SIG,
    "tfidf_wildcard_terms_batch": _wildcard_terms_sig(U32P),
    "tfidf_reader_wildcard_terms_batch": _wildcard_terms_sig(U32P),
    "tfidf_node_wildcard_terms_batch": _wildcard_terms_sig(U64P),
    "tfidf_wildcard_terms": _WILDCARD_TERMS_SINGLE_SIG,
    "tfidf_reader_wildcard_terms": _WILDCARD_TERMS_SINGLE_SIG,
    "tfidf_search_wildcard_batch": _wildcard_docs_sig(U32P),
    "tfidf_reader_search_wildcard_batch": _wildcard_docs_sig(U32P),
    "tfidf_node_search_wildcard_batch": _wildcard_docs_sig(U64P),
    "tfidf_search_wildcard": _WILDCARD_DOCS_SINGLE_SIG,
    "tfidf_reader_search_wildcard": _WILDCARD_DOCS_SINGLE_SIG,
    "tfidf_last_wildcard_stats": (C.c_int, [VP, U64P, U64P, U64P]),
    # the regex calls are shaped exactly like their wildcard twins
    "tfidf_regex_terms_batch": _wildcard_terms_sig(U32P),
    "tfidf_reader_regex_terms_batch": _wildcard_terms_sig(U32P),
    "tfidf_node_regex_terms_batch": _wildcard_terms_sig(U64P),
    "tfidf_regex_terms": _WILDCARD_TERMS_SINGLE_SIG,
    "tfidf_reader_regex_terms": _WILDCARD_TERMS_SINGLE_SIG,
    "tfidf_search_regex_batch": _wildcard_docs_sig(U32P),
    "tfidf_reader_search_regex_batch": _wildcard_docs_sig(U32P),
    "tfidf_node_search_regex_batch": _wildcard_docs_sig(U64P),
    "tfidf_search_regex": _WILDCARD_DOCS_SINGLE_SIG,
    "tfidf_reader_search_regex": _WILDCARD_DOCS_SINGLE_SIG,
    "tfidf_last_regex_stats": (C.c_int, [VP, U64P, U64P, U64P, U64P]),
    "tfidf_search_phrase_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, F32P, U32P, C.c_uint64, U64P,
                                            U64P]),
    "tfidf_reader_search_phrase_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, F32P, U32P, C.c_uint64,
                                                   U64P, U64P]),
    "tfidf_search_phrase": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, F32P, U32P, C.c_uint64, U64P]),
    "tfidf_reader_search_phrase": (C.c_int, [VP, C.c_char_p, C.c_uint64, U32P, F32P, U32P, C.c_uint64, U64P]),
    "tfidf_node_search_phrase_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U64P, F32P, U32P, C.c_uint64,
                                                 U64P, U64P]),
    "tfidf_last_phrase_stats": (C.c_int, [VP, U64P, U64P]),
    "tfidf_search_phrase_slop_batch": (C.c_int, [VP, C.c_char_p, U64P, U32P, C.c_uint32, U32P, F32P, F32P, C.c_uint64,
                                                 U64P, U64P]),
    "tfidf_reader_search_phrase_slop_batch": (C.c_int, [VP, C.c_char_p, U64P, U32P, C.c_uint32, U32P, F32P, F32P,
                                                        C.c_uint64, U64P, U64P]),
    "tfidf_search_phrase_slop": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U32P, F32P, F32P, C.c_uint64, U64P]),
    "tfidf_reader_search_phrase_slop": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U32P, F32P, F32P, C.c_uint64,
                                                  U64P]),
    "tfidf_node_search_phrase_slop_batch": (C.c_int, [VP, C.c_char_p, U64P, U32P, C.c_uint32, U64P, F32P, F32P,
                                                      C.c_uint64, U64P, U64P]),
    "tfidf_search_compound_batch": _compound_batch_sig(U32P),
    "tfidf_reader_search_compound_batch": _compound_batch_sig(U32P),
    "tfidf_node_search_compound_batch": _compound_batch_sig(U64P),
    "tfidf_search_compound": _COMPOUND_SINGLE_SIG,
    "tfidf_reader_search_compound": _COMPOUND_SINGLE_SIG,
    "tfidf_search_nested_batch": _nested_batch_sig(U32P),
    "tfidf_reader_search_nested_batch": _nested_batch_sig(U32P),
    "tfidf_node_search_nested_batch": _nested_batch_sig(U64P),
    "tfidf_search_nested": _NESTED_SINGLE_SIG,
    "tfidf_reader_search_nested": _NESTED_SINGLE_SIG,
    "tfidf_last_compound_stats": (C.c_int, [VP, U64P, U64P, U64P]),
    "tfidf_last_compound_ms": (C.c_int, [VP, F32P]),
    "tfidf_mlt_params_init": (C.c_int, [MLTP]),
    "tfidf_mlt_terms_batch": _MLT_TERMS_SIG,
    "tfidf_reader_mlt_terms_batch": _MLT_TERMS_SIG,
    "tfidf_more_like_this_batch": _MLT_BATCH_SIG,
    "tfidf_reader_more_like_this_batch": _MLT_BATCH_SIG,
    "tfidf_more_like_this": _MLT_SINGLE_SIG,
    "tfidf_reader_more_like_this": _MLT_SINGLE_SIG,
    "tfidf_last_mlt_stats": (C.c_int, [VP, U64P, U64P]),
    "tfidf_query_positive_terms": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_set_hash_attempt": (C.c_int, [VP, C.c_uint32]),
    "tfidf_get_commit_timing": (C.c_int, [VP, C.POINTER(CommitTiming)]),
    "tfidf_commit_tokenized_docs": (C.c_int, [VP, U64P, U32P]),
    "tfidf_commit_inverted_blocks": (C.c_int, [VP, U32P, U32P, U32P]),
    "tfidf_commit_inversion_shape": (C.c_int, [VP, U32P, U32P]),
    "tfidf_commit_inversion_fused": (C.c_int, [VP, U32P]),
    "tfidf_commit_host_profile": (C.c_int, [VP, C.POINTER(HostProfile)]),
    "tfidf_stats": (C.c_int, [VP, C.POINTER(IndexStats)]),
    "tfidf_search": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U32P, F32P, C.c_uint64, U64P]),
    "tfidf_search_coalesced": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U32P, F32P, C.c_uint64, U64P,
                                         C.c_uint32]),
    "tfidf_search_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, U32P, F32P, U32P]),
    "tfidf_search_batch_all": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, F32P, C.c_uint64, U64P, U64P]),
    "tfidf_reader_search_batch_all": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U32P, F32P, C.c_uint64, U64P,
                                                U64P]),
    "tfidf_last_search_ms": (C.c_int, [VP, F32P, F32P]),
    "tfidf_set_query_timing": (C.c_int, [VP, C.c_int]),
    "tfidf_search_batch_keys_device": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, C.c_uint64, VP]),
    "tfidf_search_all_keys_device": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint64, VP, C.c_uint64, U64P]),
    "tfidf_set_stream": (C.c_int, [VP, VP]),
    "tfidf_doc_keys": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_sort_names": (C.c_int, [C.c_char_p, U64P, C.c_uint64, U64P]),
    "tfidf_doc_key": (C.c_int, [VP, C.c_uint64, C.c_char_p, C.c_uint64, U64P]),
    "tfidf_doc_len": (C.c_int, [VP, C.c_uint64, U32P, U8P]),
    "tfidf_malformed_docs": (C.c_int, [VP, U64P, C.c_uint64, U64P]),
    "tfidf_doc_terms": (C.c_int, [VP, C.c_uint64, C.c_char_p, C.c_uint64, U32P, C.c_uint64, U64P]),
    "tfidf_term_df": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_vocab_size": (C.c_int, [VP, U64P]),
    "tfidf_vocab_export": (C.c_int, [VP, U64P, U32P, U32P, C.c_uint64, U64P]),
    "tfidf_vocab_export_device": (C.c_int, [VP, VP, VP, C.c_uint64, U64P]),
    "tfidf_vocab_canonicalize_device": (C.c_int, [VP, VP, C.c_uint64, VP, C.c_uint64, U64P]),
    "tfidf_set_global_stats_device": (C.c_int, [VP, VP, C.c_uint64, C.c_uint64, C.c_uint64]),
    "tfidf_vocab_partition_device": (C.c_int, [VP, C.c_uint32, VP, C.c_uint64, VP, U64P]),
    "tfidf_vocab_reduce_device": (C.c_int, [VP, VP, C.c_uint64, VP, VP]),
    "tfidf_set_global_df_device": (C.c_int, [VP, VP, C.c_uint64, C.c_uint64, C.c_uint64]),
    "tfidf_set_global_stats": (C.c_int, [VP, U64P, U64P, C.c_uint64, C.c_uint64, C.c_uint64]),
    "tfidf_clear_global_stats": (C.c_int, [VP]),
    "tfidf_term_key": (C.c_int, [C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_analyze": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_leader_merge": (C.c_int, [C.c_char_p, U64P, C.c_uint64, F64P, U64P, F64P, U64P]),
    "tfidf_synth_corpus": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, F64P, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.POINTER(VP), C.POINTER(VP), U64P]),
    # node level (csrc/tfidf_dist.hip)
    "tfidf_comm_create": (C.c_int, [C.c_int32, C.c_int32, VP, C.POINTER(VP)]),
    "tfidf_rccl_unique_id": (C.c_int, [VP]),
    "tfidf_comm_init_rccl": (C.c_int, [VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(VP)]),
    "tfidf_comm_create_inproc": (C.c_int, [C.c_int32, C.POINTER(VP)]),
    "tfidf_comm_destroy": (C.c_int, [VP]),
    "tfidf_comm_info": (C.c_int, [VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tfidf_comm_selftest": (C.c_int, [VP]),
    "tfidf_dist_global_commit": (C.c_int, [VP, VP, U64P, U64P, U64P]),
    "tfidf_dist_search": (C.c_int, [VP, VP, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, U64P, F32P, C.c_uint64,
                                    U64P]),
    "tfidf_dist_search_batch": (C.c_int, [VP, VP, C.c_uint64, C.c_char_p, U64P, C.c_uint32, C.c_uint32, U64P, F32P,
                                          U32P]),
    "tfidf_dist_shard_commit": (C.c_int, [VP, VP, U64P]),
    "tfidf_dist_shard_search": (C.c_int, [VP, VP, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_dist_search_batch_all": (C.c_int, [VP, VP, C.c_uint64, C.c_char_p, U64P, C.c_uint32, U64P, F32P, C.c_uint64,
                                              U64P, U64P]),
    "tfidf_dist_shard_search_batch": (C.c_int, [VP, VP, C.c_char_p, U64P, C.c_uint32, U64P, U64P]),
    "tfidf_dist_last_names_batch": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, F64P, C.c_uint64, U64P, U64P, U64P]),
    "tfidf_dist_last_hits": (C.c_int, [VP, U64P, F32P, C.c_uint64, U64P]),
    "tfidf_dist_last_failed": (C.c_int, [VP, U64P]),
    "tfidf_reader_open": (C.c_int, [VP, C.POINTER(VP)]),
    "tfidf_reader_close": (C.c_int, [VP]),
    "tfidf_reader_info": (C.c_int, [VP, U64P, U64P]),
    "tfidf_reader_search": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U32P, F32P, C.c_uint64, U64P]),
    "tfidf_reader_doc_key": (C.c_int, [VP, C.c_uint64, C.c_char_p, C.c_uint64, U64P]),
    "tfidf_reader_doc_keys": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, U64P]),
    "tfidf_dist_last_names": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, F64P, C.c_uint64, U64P, U64P]),
    "tfidf_node_create": (C.c_int, [VP, C.c_uint64, C.POINTER(VP)]),
    "tfidf_node_create_devices": (C.c_int, [VP, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.POINTER(VP)]),
    "tfidf_node_destroy": (C.c_int, [VP]),
    "tfidf_node_shard": (C.c_int, [VP, C.c_uint32, C.POINTER(VP), U32P]),
    "tfidf_node_add_docs": (C.c_int, [VP, C.c_int32, C.c_char_p, U64P, C.c_uint64, C.c_char_p, U64P]),
    "tfidf_node_commit": (C.c_int, [VP]),
    "tfidf_node_delete_docs": (C.c_int, [VP, C.c_int32, C.c_char_p, U64P, C.c_uint64, U64P]),
    "tfidf_node_compact": (C.c_int, [VP, U64P]),
    "tfidf_node_search": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_uint32, U64P, F32P, C.c_uint64, U64P]),
    "tfidf_node_search_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, C.c_uint32, U64P, F32P, U32P]),
    "tfidf_node_search_names": (C.c_int, [VP, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U64P, F64P,
                                          C.c_uint64, U64P, U64P]),
    "tfidf_node_search_batch_all": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U64P, F32P, C.c_uint64, U64P, U64P]),
    "tfidf_node_search_names_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U64P, U64P]),
    "tfidf_node_last_names_batch": (C.c_int, [VP, C.c_char_p, C.c_uint64, U64P, F64P, C.c_uint64, U64P, U64P, U64P]),
    "tfidf_node_doc_key": (C.c_int, [VP, C.c_uint64, C.c_char_p, C.c_uint64, U64P]),
    "tfidf_node_matches_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U64P, U64P, U64P, U32P, U32P,
                                           C.c_uint64, U64P, U64P, F32P]),
    "tfidf_node_snippets_batch": (C.c_int, [VP, C.c_char_p, U64P, C.c_uint32, U64P, U64P, C.c_uint32, VP, C.c_uint64,
                                            U64P, U64P, U64P, U32P, U32P, C.c_uint64, U64P, U64P, U64P, F32P]),
    "tfidf_node_fuzzy_terms_batch": _fuzzy_batch_sig(U64P),
    "tfidf_node_more_like_this_batch": (C.c_int, [VP, U64P, C.c_uint32, MLTP, C.c_uint32, C.c_uint32, U64P, F32P, U32P]),
    "tfidf_node_last_failed": (C.c_int, [VP, U64P]),
    "tfidf_node_stats_get": (C.c_int, [VP, VP]),
    "tfidf_device_free": (C.c_int, [C.c_int, VP]),
    "tfidf_device_copy": (C.c_int, [C.c_int, VP, VP, C.c_uint64, C.c_int]),
    "tfidf_device_copy_ms": (C.c_int, [C.c_int, VP, C.c_uint64, C.c_uint32, F32P]),
}

_lib = None


def build(jobs=8):
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", PKG_ROOT])


def load():
    """Load libtfidf.so.  Raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libtfidf.so not built at %s (run __graft_entry__.build())" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc == OK:
        return
    msg = load().tfidf_last_error().decode(errors="replace")
    if rc == E_UNSUPPORTED_QUERY:
        raise UnsupportedQuery(rc, msg)
    if rc == E_UNSUPPORTED_INPUT:
        raise UnsupportedInput(rc, msg)
    if rc == E_QUERY_SYNTAX:
        raise QuerySyntaxError(rc, msg)
    raise TfidfError(rc, msg)


def ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))
