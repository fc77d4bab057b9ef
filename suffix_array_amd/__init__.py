"""suffix_array_amd -- host-side mirror of the reference's construction interface.

The product is the C-ABI library ``libsuffix_array_amd.so`` (include/suffix_array_amd.h); this
package is the thin Python binding used by tests and bench.py.  Names, argument meaning and
error behaviour follow the reference crate for the one path that is in scope:

    SuffixArray.new / set / len / is_empty / into_parts / from_parts / unchecked_from_parts
        reference src/sa.rs:23-70, integrity check src/sa.rs:72-84
    saca(s, sa), MAX_LENGTH
        reference src/saca.rs:6-15

There is no CPU fallback: if the HIP library is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

__all__ = ["MAX_LENGTH", "saca", "SuffixArray", "SuffixArrayError", "lib", "diag_lib", "library_path", "Stats", "last_host_timing",
           "saca_batch", "workspace_bytes", "device_pci_bus_id", "saca_device_ptr", "bucket_table", "check_integrity", "last_stats", "DeviceIndex", "pack", "unpack",
           "lcp", "saca_lcp", "last_lcp_stats", "lcp_work_bytes", "lcp_device_ptr", "LcpStats",
           "lcp_set_compare_cap", "last_search_stats", "SearchStats",
           "bwt", "unbwt", "bwt_device_ptr", "unbwt_device_ptr", "bwt_work_bytes", "unbwt_work_bytes", "last_unbwt_stats",
           "unbwt_set_walk_limits", "unbwt_set_splitter_spacing", "UnbwtStats",
           "repeat_lengths", "repeat_spans", "last_repeat_stats", "repeats_work_bytes", "repeat_spans_bound",
           "repeat_lengths_device_ptr", "repeat_spans_device_ptr", "RepeatStats", "REPEATS_ALL", "REPEATS_KEEP_FIRST",
           "lpf", "lz77", "lz77_decode", "lz77_literals", "last_lz_stats", "lz_work_bytes", "lpf_device_ptr", "lz77_device_ptr", "LzStats", "LZ_LITERAL",
           "repeated_substrings", "last_substr_stats", "substrings_work_bytes", "substrings_bound", "substrings_device_ptr", "SubstrQuery", "SubstrStats",
           "SUBSTR_ALL", "SUBSTR_BY_COUNT", "SUBSTR_BY_LENGTH", "SUBSTR_BY_COVER",
           "DocSubstrQuery", "DocSubstrStats", "SUBSTR_BY_DOCS", "last_doc_substr_stats", "doc_substrings_work_bytes",
           "MatchStats", "last_match_stats", "match_work_bytes", "match_set_group_cap", "match_set_group_lanes", "match_stats_device_ptr", "match_spans_device_ptr",
           "MATCH_NONE", "MATCH_TILE",
           "DocRepeatStats", "last_doc_repeat_stats", "doc_repeats_work_bytes", "DOCREP_ANY", "DOCREP_OTHER",
           "DocsStats", "last_docs_stats", "docs_set_chunk", "docs_work_bytes", "doc_of_device_ptr", "DOC_NONE", "DOC_SAMPLES",
           "DOC_CHUNK_MIN", "DOC_CHUNK_MAX", "DOC_CHUNK_DEFAULT",
           "Not", "DocMatchStats", "last_doc_match_stats", "doc_match_set_budget", "DOC_MATCH_BUDGET_DEFAULT", "DOC_MATCH_TILE_WORDS",
           "TOKEN_DOC_OPS",
           "DocTfStats", "last_doc_tf_stats", "docs_set_topk_piece", "DOC_TOPK_MAX", "DOC_TOPK_PIECE_MIN", "DOC_TOPK_PIECE_MAX",
           "DOC_TOPK_PIECE_DEFAULT",
           "NgramStats", "last_ngram_stats", "ngram_set_stream_cap", "NGRAM_STREAM_CAP_DEFAULT",
           "ScoreStats", "ScoreResult", "last_score_stats", "score_set_group_cap", "score_work_bytes", "infgram_score_device_ptr",
           "SCORE_MAX_CONTEXT", "SCORE_GROUP_CAP_DEFAULT", "SCORE_TILE",
           "saca_u16", "MAX_TOKENS_U16", "TokenIndex", "TokStats", "last_tok_stats", "TokScoreStats", "last_tok_score_stats",
           "saca_u32", "MAX_TOKENS_U32", "TOKEN_LIMIT_U32", "TokenIndex32"]

#: reference src/saca.rs:6
MAX_LENGTH = 2**31 - 1
#: the longest 16-bit token text (sa_amd_max_tokens_u16): its byte image has at most MAX_LENGTH bytes
MAX_TOKENS_U16 = MAX_LENGTH // 2
#: the ids of a 32-bit token text lie below it (SA_AMD_TOKEN_LIMIT_U32): three bytes a token in the image
TOKEN_LIMIT_U32 = 1 << 24
#: the longest 32-bit token text (sa_amd_max_tokens_u32): its 3-byte image has at most MAX_LENGTH bytes
MAX_TOKENS_U32 = MAX_LENGTH // 3

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libsuffix_array_amd.so"
_lib: Optional[ctypes.CDLL] = None


class SuffixArrayError(RuntimeError):
    """Engine failure (the reference panics on a non-zero return of its C engine)."""

    def __init__(self, code: int, what: str):
        super().__init__(f"suffix_array_amd: {what} (status {code})")
        self.code = code


class Stats(ctypes.Structure):
    """sa_amd_stats of include/suffix_array_amd.h"""
    _fields_ = [("sigma", ctypes.c_int32), ("bits_per_symbol", ctypes.c_int32),
                ("symbols_per_key", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("sort_passes", ctypes.c_int32), ("sparse_mode", ctypes.c_int32),
                ("sorted_elements", ctypes.c_int64), ("unresolved_after_initial", ctypes.c_int64),
                ("text_rounds", ctypes.c_int32), ("top32_first", ctypes.c_int32), ("locally_sorted", ctypes.c_int64),
                ("readbacks", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LcpStats(ctypes.Structure):
    """sa_amd_lcp_stats of include/suffix_array_amd.h"""
    _fields_ = [("irreducible", ctypes.c_int64), ("compared_bytes", ctypes.c_int64), ("long_pairs", ctypes.c_int64),
                ("readbacks", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SearchStats(ctypes.Structure):
    """sa_amd_search_stats of include/suffix_array_amd.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("compared_bytes", ctypes.c_int64), ("steps", ctypes.c_int64),
                ("table_steps", ctypes.c_int64), ("route", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class UnbwtStats(ctypes.Structure):
    """sa_amd_unbwt_stats of include/suffix_array_amd.h"""
    _fields_ = [("walkers", ctypes.c_int64), ("steps", ctypes.c_int64), ("longest_walk", ctypes.c_int64),
                ("splitter_spacing", ctypes.c_int32), ("walk_launches", ctypes.c_int32), ("restarts", ctypes.c_int32),
                ("readbacks", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class RepeatStats(ctypes.Structure):
    """sa_amd_repeat_stats of include/suffix_array_amd.h"""
    _fields_ = [("longest", ctypes.c_int64), ("longest_pos", ctypes.c_int64), ("lcp_sum", ctypes.c_int64),
                ("distinct_substrings", ctypes.c_int64), ("spans", ctypes.c_int64), ("covered_bytes", ctypes.c_int64),
                ("flagged", ctypes.c_int64), ("readbacks", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class LzStats(ctypes.Structure):
    """sa_amd_lz_stats of include/suffix_array_amd.h"""
    _fields_ = [("phrases", ctypes.c_int64), ("literals", ctypes.c_int64), ("longest", ctypes.c_int64), ("longest_pos", ctypes.c_int64),
                ("unresolved", ctypes.c_int64), ("hierarchy_steps", ctypes.c_int64), ("hierarchy_max", ctypes.c_int64),
                ("walkers", ctypes.c_int64), ("walk_steps", ctypes.c_int64), ("walk_launches", ctypes.c_int32),
                ("restarts", ctypes.c_int32), ("splitter_spacing", ctypes.c_int32), ("readbacks", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SubstrQuery(ctypes.Structure):
    """sa_amd_substr_query of include/suffix_array_amd.h"""
    _fields_ = [("min_len", ctypes.c_int32), ("max_len", ctypes.c_int32), ("min_count", ctypes.c_int32), ("order", ctypes.c_int32),
                ("k", ctypes.c_int64)]


class SubstrStats(ctypes.Structure):
    """sa_amd_substr_stats of include/suffix_array_amd.h"""
    _fields_ = [("nodes", ctypes.c_int64), ("selected", ctypes.c_int64), ("distinct_all", ctypes.c_int64),
                ("distinct_selected", ctypes.c_int64), ("unresolved", ctypes.c_int64), ("far_steps", ctypes.c_int64),
                ("far_max", ctypes.c_int64), ("sorted", ctypes.c_int64), ("select_passes", ctypes.c_int32), ("readbacks", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


#: orders of ``repeated_substrings`` (SA_AMD_SUBSTR_* of include/suffix_array_amd.h)
SUBSTR_ALL, SUBSTR_BY_COUNT, SUBSTR_BY_LENGTH, SUBSTR_BY_COVER = 0, 1, 2, 3
#: the order ``DeviceIndex.doc_substrings`` adds: by document frequency (SA_AMD_SUBSTR_BY_DOCS)
SUBSTR_BY_DOCS = 4


class DocSubstrQuery(ctypes.Structure):
    """sa_amd_doc_substr_query of include/suffix_array_amd.h"""
    _fields_ = [("min_len", ctypes.c_int32), ("max_len", ctypes.c_int32), ("min_count", ctypes.c_int32), ("order", ctypes.c_int32),
                ("k", ctypes.c_int64), ("min_docs", ctypes.c_int64)]


class DocSubstrStats(ctypes.Structure):
    """sa_amd_doc_substr_stats of include/suffix_array_amd.h"""
    _fields_ = [("nodes", ctypes.c_int64), ("selected", ctypes.c_int64), ("distinct_selected", ctypes.c_int64),
                ("df_sum", ctypes.c_int64), ("max_df", ctypes.c_int64), ("pairs", ctypes.c_int64), ("rmq_far", ctypes.c_int64),
                ("rmq_steps", ctypes.c_int64), ("rmq_max", ctypes.c_int64), ("sorted", ctypes.c_int64),
                ("select_passes", ctypes.c_int32), ("readbacks", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MatchStats(ctypes.Structure):
    """sa_amd_match_stats of include/suffix_array_amd.h"""
    _fields_ = [("positions", ctypes.c_int64), ("matched", ctypes.c_int64), ("longest", ctypes.c_int64), ("longest_pos", ctypes.c_int64),
                ("ml_sum", ctypes.c_int64), ("long_positions", ctypes.c_int64), ("compared_bytes", ctypes.c_int64), ("steps", ctypes.c_int64),
                ("spans", ctypes.c_int64), ("covered_bytes", ctypes.c_int64), ("flagged", ctypes.c_int64), ("route_long", ctypes.c_int32),
                ("readbacks", ctypes.c_int32), ("group_lanes", ctypes.c_int32), ("group_cap", ctypes.c_int32), ("tile", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class DocsStats(ctypes.Structure):
    """sa_amd_docs_stats of include/suffix_array_amd.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("occ_sum", ctypes.c_int64), ("units", ctypes.c_int64), ("df_sum", ctypes.c_int64),
                ("slots_scanned", ctypes.c_int64), ("chunk", ctypes.c_int32), ("readbacks", ctypes.c_int32), ("listed", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class DocMatchStats(ctypes.Structure):
    """sa_amd_doc_match_stats of include/suffix_array_amd_docmatch.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("clauses", ctypes.c_int64), ("queries", ctypes.c_int64), ("occ_sum", ctypes.c_int64),
                ("units", ctypes.c_int64), ("marks", ctypes.c_int64), ("bitmap_words", ctypes.c_int64), ("slabs", ctypes.c_int64),
                ("df_sum", ctypes.c_int64), ("budget", ctypes.c_int64), ("chunk", ctypes.c_int32), ("readbacks", ctypes.c_int32),
                ("listed", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class Not:
    """A negated clause of ``doc_match`` / ``doc_match_list``: ``Not(b"x")`` holds the documents without ``x``,
    ``Not([b"x", b"y"])`` those with neither."""
    __slots__ = ("clause",)

    def __init__(self, clause):
        if isinstance(clause, Not):
            raise TypeError("Not(Not(...)): pass the clause itself")
        self.clause = clause

    def __repr__(self):
        return f"Not({self.clause!r})"


class DocTfStats(ctypes.Structure):
    """sa_amd_doc_tf_stats of include/suffix_array_amd.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("occ_sum", ctypes.c_int64), ("df_sum", ctypes.c_int64), ("tf_sum", ctypes.c_int64),
                ("table_loads", ctypes.c_int64), ("topk_entries", ctypes.c_int64), ("pieces", ctypes.c_int64), ("rounds", ctypes.c_int32),
                ("k", ctypes.c_int32), ("piece", ctypes.c_int32), ("chunk", ctypes.c_int32), ("readbacks", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class NgramStats(ctypes.Structure):
    """sa_amd_ngram_stats of include/suffix_array_amd.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("range_searches", ctypes.c_int64), ("compared_bytes", ctypes.c_int64),
                ("stream_slots", ctypes.c_int64), ("search_slots", ctypes.c_int64), ("stream_queries", ctypes.c_int64),
                ("search_queries", ctypes.c_int64), ("empty_queries", ctypes.c_int64), ("entries", ctypes.c_int64),
                ("stream_cap", ctypes.c_int32), ("readbacks", ctypes.c_int32), ("backoff", ctypes.c_int32), ("passes", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TokStats(ctypes.Structure):
    """sa_amd_tok_stats of include/suffix_array_amd.h"""
    _fields_ = [("patterns", ctypes.c_int64), ("range_searches", ctypes.c_int64), ("compared_tokens", ctypes.c_int64),
                ("stream_slots", ctypes.c_int64), ("search_slots", ctypes.c_int64), ("stream_queries", ctypes.c_int64),
                ("search_queries", ctypes.c_int64), ("empty_queries", ctypes.c_int64), ("entries", ctypes.c_int64),
                ("stream_cap", ctypes.c_int32), ("readbacks", ctypes.c_int32), ("backoff", ctypes.c_int32), ("passes", ctypes.c_int32),
                ("image_ms", ctypes.c_double), ("build_ms", ctypes.c_double), ("compact_ms", ctypes.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ScoreStats(ctypes.Structure):
    """sa_amd_score_stats of include/suffix_array_amd.h"""
    _fields_ = [("positions", ctypes.c_int64), ("documents", ctypes.c_int64), ("group_searches", ctypes.c_int64),
                ("long_searches", ctypes.c_int64), ("next_lookups", ctypes.c_int64), ("compared_bytes", ctypes.c_int64),
                ("long_positions", ctypes.c_int64), ("zero_positions", ctypes.c_int64), ("group_cap", ctypes.c_int32),
                ("readbacks", ctypes.c_int32)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["range_searches"] = d["group_searches"] + d["long_searches"]
        return d


class TokScoreStats(ctypes.Structure):
    """sa_amd_tok_score_stats of include/suffix_array_amd.h: the fields of ``ScoreStats``, ``compared_tokens`` for ``compared_bytes``"""
    _fields_ = [(("compared_tokens" if name == "compared_bytes" else name), ctype) for name, ctype in ScoreStats._fields_]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["range_searches"] = d["group_searches"] + d["long_searches"]
        return d


#: the longest context ``infgram_score`` takes (SA_AMD_SCORE_MAX_CONTEXT: what a tile stages)
SCORE_MAX_CONTEXT = 4096
#: context bytes the lane groups of ``infgram_score`` probe before a position goes to the one-wave path (kernels/score.hpp)
SCORE_GROUP_CAP_DEFAULT = 64
#: query positions per workgroup of ``infgram_score``
SCORE_TILE = 256


class ScoreResult:
    """What ``infgram_score`` returns, arrays over the positions of the query: ``s`` (the back-off length), ``lo`` / ``hi`` /
    ``at_end`` (the context's range and at-end flag) and ``nlo`` / ``nhi`` (the sub-range of the context followed by the byte
    that is there)."""

    def __init__(self, s, lo, hi, at_end, nlo, nhi):
        self.s, self.lo, self.hi, self.at_end, self.nlo, self.nhi = s, lo, hi, at_end, nlo, nhi

    def __iter__(self):
        return iter((self.s, self.lo, self.hi, self.at_end, self.nlo, self.nhi))

    def __len__(self):
        return int(self.s.size)

    def counts(self):
        """-> ``(count, total)`` int64: occurrences of the context followed by the byte, and followed by any byte"""
        cnt = self.nhi.astype(np.int64) - self.nlo.astype(np.int64)
        den = self.hi.astype(np.int64) - self.lo.astype(np.int64) - self.at_end.astype(np.int64)
        return cnt, den

    def log2_prob(self) -> np.ndarray:
        """float64 ``log2`` of the model's probability of every byte; ``-inf`` where the count or the denominator is 0"""
        cnt, den = self.counts()
        out = np.full(cnt.size, -np.inf, dtype=np.float64)
        ok = (cnt > 0) & (den > 0)
        out[ok] = np.log2(cnt[ok].astype(np.float64)) - np.log2(den[ok].astype(np.float64))
        return out

    def doc_bits(self, doc_offsets=None):
        """-> ``(bits, zeros)`` per document of ``doc_offsets`` (``None``: one document): the sum of ``-log2 p`` over the
        positions with ``p > 0`` and the number of positions with ``p = 0`` -- how those are smoothed is the caller's policy"""
        lp = self.log2_prob()
        off = np.array([0, lp.size], dtype=np.int64) if doc_offsets is None else np.ascontiguousarray(doc_offsets, dtype=np.int64)
        fin = np.isfinite(lp)
        cb = np.concatenate(([0.0], np.cumsum(np.where(fin, -lp, 0.0))))
        cz = np.concatenate(([0], np.cumsum(~fin))).astype(np.int64)
        return cb[off[1:]] - cb[off[:-1]], cz[off[1:]] - cz[off[:-1]]


#: slots up to which ``next_bytes`` / ``infgram`` stream a range instead of searching its run starts (kernels/ngram.hpp)
NGRAM_STREAM_CAP_DEFAULT = 1024


class DocRepeatStats(ctypes.Structure):
    """sa_amd_doc_repeat_stats of include/suffix_array_amd.h"""
    _fields_ = [("members", ctypes.c_int64), ("flagged", ctypes.c_int64), ("spans", ctypes.c_int64), ("covered_bytes", ctypes.c_int64),
                ("docs_touched", ctypes.c_int64), ("readbacks", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


#: the document of a position behind the text (SA_AMD_DOC_NONE of include/suffix_array_amd.h); equal to ``MATCH_NONE``
DOC_NONE = 0xFFFFFFFF
#: entries of the sampled top level of the offset table a workgroup stages (kernels/docs.hpp)
DOC_SAMPLES = 8192
#: slots of a unit of ``doc_search`` / ``doc_list``: the clamp of ``docs_set_chunk`` and the default (kernels/docs.hpp)
DOC_CHUNK_MIN = 64
DOC_CHUNK_MAX = 1 << 20
DOC_CHUNK_DEFAULT = 4096
#: bytes of clause bitmaps a slab of ``doc_match`` queries may hold by default (host/doc_match.hpp), and the bitmap words one
#: wave combines (kernels/doc_match.hpp): 32 documents a word
DOC_MATCH_BUDGET_DEFAULT = 256 << 20
DOC_MATCH_TILE_WORDS = 256
#: the document calls of include/sa_amd_tokdocs.h, each behind ``sa_amd_tok_index_`` and ``sa_amd_tok32_index_``
TOKEN_DOC_OPS = ("set_documents", "set_documents_by_separator", "doc_offsets", "doc_of", "doc_search", "doc_list", "doc_match", "doc_match_list")

#: the largest ``k`` of ``doc_topk`` (SA_AMD_DOC_TOPK_MAX of include/suffix_array_amd.h)
DOC_TOPK_MAX = 1024
#: keys of a piece of the top-k reduction: the clamp of ``docs_set_topk_piece`` and the default (kernels/doc_tf.hpp)
DOC_TOPK_PIECE_MIN = 64
DOC_TOPK_PIECE_MAX = 4096
DOC_TOPK_PIECE_DEFAULT = 1024

#: ``pos`` of a query position none of whose bytes occurs in the text (SA_AMD_MATCH_NONE of include/suffix_array_amd.h)
MATCH_NONE = 0xFFFFFFFF
#: query positions one workgroup of the group path owns (kernels/match.hpp)
MATCH_TILE = 256

#: the source of a literal phrase, and of a position without an earlier copy (SA_AMD_LZ_LITERAL of include/suffix_array_amd.h)
LZ_LITERAL = 0xFFFFFFFF

#: span modes of ``repeat_spans_device_ptr`` (SA_AMD_REPEATS_* of include/suffix_array_amd.h)
REPEATS_ALL = 0
REPEATS_KEEP_FIRST = 1
#: scopes of ``DeviceIndex.doc_repeat_spans`` (SA_AMD_DOCREP_* of include/suffix_array_amd.h): a copy anywhere / in another document
DOCREP_ANY = 0
DOCREP_OTHER = 1


def library_path() -> str:
    return os.path.join(_HERE, _LIB_NAME)


def lib() -> ctypes.CDLL:
    """Load the C-ABI library (built in-tree by __graft_entry__.build()); fail loudly if absent."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = ctypes.CDLL(path)
        c_u8p, c_vp = ctypes.c_void_p, ctypes.c_void_p
        L.sa_amd_max_length.restype = ctypes.c_int32
        L.sa_amd_divsufsort.argtypes = [c_u8p, c_vp, ctypes.c_int32]
        L.sa_amd_divsufsort.restype = ctypes.c_int32
        L.sa_amd_saca_u8.argtypes = [c_u8p, c_vp, ctypes.c_int32]
        L.sa_amd_saca_u8.restype = ctypes.c_int32
        L.sa_amd_saca_batch.argtypes = [c_vp, c_vp, c_vp, c_vp, ctypes.c_int32, c_vp]
        L.sa_amd_saca_batch.restype = ctypes.c_int32
        L.sa_amd_workspace_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_workspace_bytes.restype = ctypes.c_int64
        L.sa_amd_saca_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, c_vp]
        L.sa_amd_saca_device.restype = ctypes.c_int32
        L.sa_amd_device_count.restype = ctypes.c_int32
        L.sa_amd_device_pci_bus_id.argtypes = [ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
        L.sa_amd_device_pci_bus_id.restype = ctypes.c_int32
        L.sa_amd_bucket_table_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_bucket_table_device.restype = ctypes.c_int32
        L.sa_amd_last_stats.argtypes = [c_vp]
        L.sa_amd_index_create.argtypes = [c_vp, ctypes.c_int32, c_vp, ctypes.POINTER(ctypes.c_void_p)]
        L.sa_amd_index_create.restype = ctypes.c_int32
        L.sa_amd_index_destroy.argtypes = [c_vp]
        L.sa_amd_index_destroy.restype = None
        for fn in ("sa_amd_index_sa", "sa_amd_index_buckets"):
            getattr(L, fn).argtypes = [c_vp, c_vp]
            getattr(L, fn).restype = ctypes.c_int32
        L.sa_amd_index_check_integrity.argtypes = [c_vp]
        L.sa_amd_index_check_integrity.restype = ctypes.c_int32
        L.sa_amd_index_search.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp]
        L.sa_amd_index_search.restype = ctypes.c_int32
        L.sa_amd_pack_bound.argtypes = [ctypes.c_int64]
        L.sa_amd_pack_bound.restype = ctypes.c_int64
        L.sa_amd_pack.argtypes = [c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_pack.restype = ctypes.c_int32
        L.sa_amd_unpack.argtypes = [c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_unpack.restype = ctypes.c_int32
        L.sa_amd_bucket_table.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_bucket_table.restype = ctypes.c_int32
        L.sa_amd_saca_u8_buckets.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp]
        L.sa_amd_saca_u8_buckets.restype = ctypes.c_int32
        L.sa_amd_check_integrity.argtypes = [c_vp, ctypes.c_int32, c_vp, ctypes.c_int64]
        L.sa_amd_check_integrity.restype = ctypes.c_int32
        L.sa_amd_last_stats.restype = None
        L.sa_amd_strerror.argtypes = [ctypes.c_int32]
        L.sa_amd_strerror.restype = ctypes.c_char_p
        L.sa_amd_version.restype = ctypes.c_char_p
        L.sa_amd_profile_begin.restype = None
        L.sa_amd_profile_end.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32]
        L.sa_amd_profile_end.restype = ctypes.c_int32
        L.sa_amd_profile_kernel_name.argtypes = [ctypes.c_int32]
        L.sa_amd_profile_kernel_name.restype = ctypes.c_char_p
        L.sa_amd_last_host_timing.argtypes = [c_vp, ctypes.c_int32]
        L.sa_amd_last_host_timing.restype = ctypes.c_int32
        L.sa_amd_profile_begin_classes.argtypes = [ctypes.c_uint64]
        L.sa_amd_profile_begin_classes.restype = None
        L.sa_amd_check_integrity_device.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_check_integrity_device.restype = ctypes.c_int32
        L.sa_amd_check_integrity_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_check_integrity_work_bytes.restype = ctypes.c_int64
        L.sa_amd_lcp_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_lcp_work_bytes.restype = ctypes.c_int64
        L.sa_amd_lcp_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_lcp_device.restype = ctypes.c_int32
        L.sa_amd_lcp.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_lcp.restype = ctypes.c_int32
        L.sa_amd_saca_u8_lcp.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp]
        L.sa_amd_saca_u8_lcp.restype = ctypes.c_int32
        L.sa_amd_index_lcp.argtypes = [c_vp, c_vp]
        L.sa_amd_index_lcp.restype = ctypes.c_int32
        L.sa_amd_last_lcp_stats.argtypes = [c_vp]
        L.sa_amd_last_lcp_stats.restype = None
        L.sa_amd_lcp_set_compare_cap.argtypes = [ctypes.c_int32]
        L.sa_amd_lcp_set_compare_cap.restype = ctypes.c_int32
        L.sa_amd_index_enable_lcp.argtypes = [c_vp]
        L.sa_amd_index_enable_lcp.restype = ctypes.c_int32
        L.sa_amd_last_search_stats.argtypes = [c_vp]
        L.sa_amd_last_search_stats.restype = None
        L.sa_amd_bwt_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_bwt_work_bytes.restype = ctypes.c_int64
        L.sa_amd_bwt_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_bwt_device.restype = ctypes.c_int32
        L.sa_amd_bwt.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, c_vp]
        L.sa_amd_bwt.restype = ctypes.c_int32
        L.sa_amd_index_bwt.argtypes = [c_vp, c_vp, c_vp]
        L.sa_amd_index_bwt.restype = ctypes.c_int32
        L.sa_amd_unbwt_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_unbwt_work_bytes.restype = ctypes.c_int64
        L.sa_amd_unbwt_device.argtypes = [c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_unbwt_device.restype = ctypes.c_int32
        L.sa_amd_unbwt.argtypes = [c_vp, ctypes.c_int32, ctypes.c_int32, c_vp]
        L.sa_amd_unbwt.restype = ctypes.c_int32
        L.sa_amd_last_unbwt_stats.argtypes = [c_vp]
        L.sa_amd_last_unbwt_stats.restype = None
        L.sa_amd_unbwt_set_walk_limits.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.sa_amd_unbwt_set_walk_limits.restype = None
        L.sa_amd_unbwt_set_splitter_spacing.argtypes = [ctypes.c_int32]
        L.sa_amd_unbwt_set_splitter_spacing.restype = ctypes.c_int32
        L.sa_amd_repeats_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_repeats_work_bytes.restype = ctypes.c_int64
        L.sa_amd_repeat_spans_bound.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.sa_amd_repeat_spans_bound.restype = ctypes.c_int64
        L.sa_amd_repeat_lengths_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_repeat_lengths_device.restype = ctypes.c_int32
        L.sa_amd_repeat_spans_device.argtypes = [c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64,
                                                 c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_repeat_spans_device.restype = ctypes.c_int32
        L.sa_amd_repeat_lengths.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_repeat_lengths.restype = ctypes.c_int32
        L.sa_amd_repeat_spans.argtypes = [c_vp, ctypes.c_int32, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_repeat_spans.restype = ctypes.c_int32
        L.sa_amd_index_repeat_lengths.argtypes = [c_vp, c_vp]
        L.sa_amd_index_repeat_lengths.restype = ctypes.c_int32
        L.sa_amd_index_repeat_spans.argtypes = [c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_repeat_spans.restype = ctypes.c_int32
        L.sa_amd_last_repeat_stats.argtypes = [c_vp]
        L.sa_amd_last_repeat_stats.restype = None
        L.sa_amd_lz_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_lz_work_bytes.restype = ctypes.c_int64
        L.sa_amd_lpf_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_lpf_device.restype = ctypes.c_int32
        L.sa_amd_lz77_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_lz77_device.restype = ctypes.c_int32
        L.sa_amd_lpf.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, c_vp]
        L.sa_amd_lpf.restype = ctypes.c_int32
        L.sa_amd_lz77.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_lz77.restype = ctypes.c_int32
        L.sa_amd_index_lpf.argtypes = [c_vp, c_vp, c_vp]
        L.sa_amd_index_lpf.restype = ctypes.c_int32
        L.sa_amd_index_lz77.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_lz77.restype = ctypes.c_int32
        L.sa_amd_last_lz_stats.argtypes = [c_vp]
        L.sa_amd_last_lz_stats.restype = None
        L.sa_amd_substrings_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_substrings_work_bytes.restype = ctypes.c_int64
        L.sa_amd_substrings_bound.argtypes = [ctypes.c_int32]
        L.sa_amd_substrings_bound.restype = ctypes.c_int64
        L.sa_amd_substrings_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_substrings_device.restype = ctypes.c_int32
        L.sa_amd_substrings.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_substrings.restype = ctypes.c_int32
        L.sa_amd_index_substrings.argtypes = [c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_substrings.restype = ctypes.c_int32
        L.sa_amd_last_substr_stats.argtypes = [c_vp]
        L.sa_amd_last_substr_stats.restype = None
        L.sa_amd_doc_substrings_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_doc_substrings_work_bytes.restype = ctypes.c_int64
        L.sa_amd_index_doc_substrings.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_doc_substrings.restype = ctypes.c_int32
        L.sa_amd_last_doc_substr_stats.argtypes = [c_vp]
        L.sa_amd_last_doc_substr_stats.restype = None
        L.sa_amd_match_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_match_work_bytes.restype = ctypes.c_int64
        L.sa_amd_index_match_stats.argtypes = [c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_index_match_stats.restype = ctypes.c_int32
        L.sa_amd_index_match_stats_device.argtypes = [c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_match_stats_device.restype = ctypes.c_int32
        L.sa_amd_index_match_spans.argtypes = [c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_match_spans.restype = ctypes.c_int32
        L.sa_amd_index_match_spans_device.argtypes = [c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, c_vp,
                                                      ctypes.c_int64, c_vp]
        L.sa_amd_index_match_spans_device.restype = ctypes.c_int32
        L.sa_amd_last_match_stats.argtypes = [c_vp]
        L.sa_amd_last_match_stats.restype = None
        L.sa_amd_match_set_group_cap.argtypes = [ctypes.c_int32]
        L.sa_amd_match_set_group_cap.restype = ctypes.c_int32
        L.sa_amd_match_set_group_lanes.argtypes = [ctypes.c_int32]
        L.sa_amd_match_set_group_lanes.restype = ctypes.c_int32
        L.sa_amd_docs_work_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_docs_work_bytes.restype = ctypes.c_int64
        L.sa_amd_index_set_documents.argtypes = [c_vp, c_vp, ctypes.c_int64]
        L.sa_amd_index_set_documents.restype = ctypes.c_int32
        L.sa_amd_index_doc_of.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_doc_of.restype = ctypes.c_int32
        L.sa_amd_index_doc_of_device.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp]
        L.sa_amd_index_doc_of_device.restype = ctypes.c_int32
        L.sa_amd_index_doc_search.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_index_doc_search.restype = ctypes.c_int32
        L.sa_amd_index_doc_list.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_doc_list.restype = ctypes.c_int32
        L.sa_amd_index_doc_match.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_index_doc_match.restype = ctypes.c_int32
        L.sa_amd_index_doc_match_list.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.c_int32, c_vp, c_vp,
                                                  ctypes.c_int64, c_vp]
        L.sa_amd_index_doc_match_list.restype = ctypes.c_int32
        L.sa_amd_last_doc_match_stats.argtypes = [c_vp]
        L.sa_amd_last_doc_match_stats.restype = None
        L.sa_amd_doc_match_set_budget.argtypes = [ctypes.c_int64]
        L.sa_amd_doc_match_set_budget.restype = ctypes.c_int64
        L.sa_amd_doc_repeats_work_bytes.argtypes = [ctypes.c_int32, ctypes.c_int64]
        L.sa_amd_doc_repeats_work_bytes.restype = ctypes.c_int64
        L.sa_amd_index_doc_repeat_spans.argtypes = [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, c_vp]
        L.sa_amd_index_doc_repeat_spans.restype = ctypes.c_int32
        L.sa_amd_last_doc_repeat_stats.argtypes = [c_vp]
        L.sa_amd_last_doc_repeat_stats.restype = None
        L.sa_amd_last_docs_stats.argtypes = [c_vp]
        L.sa_amd_last_docs_stats.restype = None
        L.sa_amd_docs_set_chunk.argtypes = [ctypes.c_int32]
        L.sa_amd_docs_set_chunk.restype = ctypes.c_int32
        L.sa_amd_index_enable_doc_freq.argtypes = [c_vp]
        L.sa_amd_index_enable_doc_freq.restype = ctypes.c_int32
        L.sa_amd_index_doc_tf.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_doc_tf.restype = ctypes.c_int32
        L.sa_amd_index_doc_topk.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp]
        L.sa_amd_index_doc_topk.restype = ctypes.c_int32
        L.sa_amd_last_doc_tf_stats.argtypes = [c_vp]
        L.sa_amd_last_doc_tf_stats.restype = None
        L.sa_amd_index_next_bytes.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_next_bytes.restype = ctypes.c_int32
        L.sa_amd_index_infgram.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_infgram.restype = ctypes.c_int32
        L.sa_amd_last_ngram_stats.argtypes = [c_vp]
        L.sa_amd_last_ngram_stats.restype = None
        L.sa_amd_ngram_set_stream_cap.argtypes = [ctypes.c_int32]
        L.sa_amd_ngram_set_stream_cap.restype = ctypes.c_int32
        L.sa_amd_index_infgram_score.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp,
                                                 c_vp, c_vp, c_vp]
        L.sa_amd_index_infgram_score.restype = ctypes.c_int32
        L.sa_amd_index_infgram_score_device.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp,
                                                        c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_index_infgram_score_device.restype = ctypes.c_int32
        L.sa_amd_score_work_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
        L.sa_amd_score_work_bytes.restype = ctypes.c_int64
        L.sa_amd_last_score_stats.argtypes = [c_vp]
        L.sa_amd_last_score_stats.restype = None
        L.sa_amd_score_set_group_cap.argtypes = [ctypes.c_int32]
        L.sa_amd_score_set_group_cap.restype = ctypes.c_int32
        L.sa_amd_docs_set_topk_piece.argtypes = [ctypes.c_int32]
        L.sa_amd_docs_set_topk_piece.restype = ctypes.c_int32
        L.sa_amd_max_tokens_u16.argtypes = []
        L.sa_amd_max_tokens_u16.restype = ctypes.c_int32
        L.sa_amd_saca_u16.argtypes = [c_vp, c_vp, ctypes.c_int32]
        L.sa_amd_saca_u16.restype = ctypes.c_int32
        L.sa_amd_tok_index_create.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_tok_index_create.restype = ctypes.c_int32
        L.sa_amd_tok_index_destroy.argtypes = [c_vp]
        L.sa_amd_tok_index_destroy.restype = None
        L.sa_amd_tok_index_sa.argtypes = [c_vp, c_vp]
        L.sa_amd_tok_index_sa.restype = ctypes.c_int32
        L.sa_amd_tok_index_search.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp]
        L.sa_amd_tok_index_search.restype = ctypes.c_int32
        L.sa_amd_tok_index_next_tokens.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_tok_index_next_tokens.restype = ctypes.c_int32
        L.sa_amd_tok_index_infgram.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                               c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_tok_index_infgram.restype = ctypes.c_int32
        L.sa_amd_last_tok_stats.argtypes = [c_vp]
        L.sa_amd_last_tok_stats.restype = None
        L.sa_amd_tok_index_infgram_score.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp,
                                                     c_vp, c_vp, c_vp, c_vp]
        L.sa_amd_tok_index_infgram_score.restype = ctypes.c_int32
        L.sa_amd_last_tok_score_stats.argtypes = [c_vp]
        L.sa_amd_last_tok_score_stats.restype = None
        # include/sa_amd_tokdocs.h: the document calls of the byte index on the token indexes
        L.sa_amd_tok_index_set_documents.argtypes = [c_vp, c_vp, ctypes.c_int64]
        L.sa_amd_tok_index_set_documents_by_separator.argtypes = [c_vp, ctypes.c_uint32, c_vp]
        L.sa_amd_tok_index_doc_offsets.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_tok_index_doc_of.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_tok_index_doc_search.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_tok_index_doc_list.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_int64, c_vp]
        L.sa_amd_tok_index_doc_match.argtypes = L.sa_amd_index_doc_match.argtypes
        L.sa_amd_tok_index_doc_match_list.argtypes = L.sa_amd_index_doc_match_list.argtypes
        for op in TOKEN_DOC_OPS:
            getattr(L, "sa_amd_tok_index_" + op).restype = ctypes.c_int32
        for u16_name, u32_name in (("sa_amd_max_tokens_u16", "sa_amd_max_tokens_u32"), ("sa_amd_saca_u16", "sa_amd_saca_u32")) + tuple(
                ("sa_amd_tok_index_" + op, "sa_amd_tok32_index_" + op)
                for op in ("create", "destroy", "sa", "search", "next_tokens", "infgram", "infgram_score") + TOKEN_DOC_OPS):
            u16_fn, u32_fn = getattr(L, u16_name), getattr(L, u32_name)       # (the signatures are the u16 ones with uint32_t tokens)
            u32_fn.argtypes, u32_fn.restype = u16_fn.argtypes, u16_fn.restype
        _lib = L
    return _lib


_diag: Optional[ctypes.CDLL] = None


def diag_lib() -> ctypes.CDLL:
    """libsuffix_array_amd_diag.so (csrc/sa_diag.h): the same sources built with -DSA_AMD_DIAG -- primitive test hooks,
    phase stamps and the timing ablations.  For tests/ and tools/ only; nothing in the product path loads it."""
    global _diag
    if _diag is None:
        path = os.path.join(_HERE, "libsuffix_array_amd_diag.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: run __graft_entry__.build()")
        L = ctypes.CDLL(path)
        c_vp = ctypes.c_void_p
        L.sa_amd_test_sort_pairs.argtypes = [c_vp, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        L.sa_amd_test_sort_pairs.restype = ctypes.c_int32
        L.sa_amd_test_sort_pairs32.argtypes = [c_vp, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        L.sa_amd_test_sort_pairs32.restype = ctypes.c_int32
        L.sa_amd_test_sort_pairs_flags.argtypes = [c_vp, c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp]
        L.sa_amd_test_sort_pairs_flags.restype = ctypes.c_int32
        L.sa_amd_debug_head_flags.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_head_flags.restype = ctypes.c_int32
        L.sa_amd_debug_round_flags.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_round_flags.restype = ctypes.c_int32
        L.sa_amd_debug_fill_blocks.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_fill_blocks.restype = ctypes.c_int32
        L.sa_amd_last_stats.argtypes = [c_vp]
        L.sa_amd_test_sample_sort64.argtypes = [c_vp, c_vp, ctypes.c_int64, ctypes.c_int32, c_vp]
        L.sa_amd_test_sample_sort64.restype = ctypes.c_int32
        L.sa_amd_test_bucket_sort32.argtypes = [c_vp, c_vp, ctypes.c_int64, ctypes.c_int32, c_vp]
        L.sa_amd_test_bucket_sort32.restype = ctypes.c_int32
        L.sa_amd_test_lz_nsv.argtypes = [c_vp, ctypes.c_int64, c_vp, c_vp, c_vp]
        L.sa_amd_test_lz_nsv.restype = ctypes.c_int32
        L.sa_amd_test_build_keys.argtypes = [c_vp, ctypes.c_int32, c_vp, c_vp, c_vp]
        L.sa_amd_test_build_keys.restype = ctypes.c_int32
        L.sa_amd_debug_phase_cycles.argtypes = [c_vp, ctypes.c_int32]
        L.sa_amd_debug_phase_cycles.restype = ctypes.c_int32
        L.sa_amd_debug_group_sort_stamps.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_group_sort_stamps.restype = ctypes.c_int32
        L.sa_amd_debug_rr_count_stamps.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_rr_count_stamps.restype = ctypes.c_int32
        L.sa_amd_debug_sort_variant_count.restype = ctypes.c_int32
        L.sa_amd_debug_sort_variant_name.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_sort_variant_name.restype = ctypes.c_char_p
        L.sa_amd_saca_u8.argtypes = [c_vp, c_vp, ctypes.c_int32]
        L.sa_amd_saca_u8.restype = ctypes.c_int32
        L.sa_amd_saca_device.argtypes = [c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, c_vp]
        L.sa_amd_saca_device.restype = ctypes.c_int32
        L.sa_amd_workspace_bytes.argtypes = [ctypes.c_int32]
        L.sa_amd_workspace_bytes.restype = ctypes.c_int64
        L.sa_amd_version.restype = ctypes.c_char_p
        _diag = L
    return _diag


def device_pci_bus_id(device: int = 0) -> str:
    """PCI address of HIP device `device` ("0000:c1:00.0"): which physical GPU an ordinal is"""
    buf = ctypes.create_string_buffer(64)
    _check(lib().sa_amd_device_pci_bus_id(int(device), buf, 64))
    return buf.value.decode()


def _check(code: int) -> None:
    if code != 0:
        raise SuffixArrayError(code, lib().sa_amd_strerror(code).decode())


def _as_u8(s) -> np.ndarray:
    if isinstance(s, np.ndarray):
        if s.dtype != np.uint8 or not s.flags.c_contiguous:
            raise TypeError("text must be a contiguous uint8 array")
        return s
    return np.frombuffer(bytes(s), dtype=np.uint8) if len(s) else np.zeros(0, dtype=np.uint8)


def saca(s, sa: np.ndarray) -> None:
    """``pub fn saca(s: &[u8], sa: &mut [u32])`` -- reference src/saca.rs:9-15.

    ``sa`` is a caller-owned uint32 array of ``len(s) + 1`` entries whose prior contents are
    irrelevant; on return ``sa[0] == len(s)`` and ``sa[1:]`` holds the sorted suffix offsets.
    The reference's two ``assert!``s (src/saca.rs:10-11) are AssertionErrors here.
    """
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH                       # src/saca.rs:10
    assert t.size + 1 == sa.size                      # src/saca.rs:11
    if sa.dtype != np.uint32 or not sa.flags.c_contiguous or not sa.flags.writeable:
        raise TypeError("sa must be a writable contiguous uint32 array")
    _check(lib().sa_amd_saca_u8(t.ctypes.data, sa.ctypes.data, t.size))


def divsufsort(s, sa: np.ndarray) -> None:
    """The C engine's own signature (n int32 entries, no sentinel) -- call site reference src/saca.rs:14."""
    t = _as_u8(s)
    assert t.size == sa.size and sa.dtype == np.int32
    _check(lib().sa_amd_divsufsort(t.ctypes.data, sa.ctypes.data, t.size))


def saca_batch(texts, devices=None):
    """Independent texts, one device each; returns the list of uint32 arrays."""
    ts = [_as_u8(t) for t in texts]
    cnt = len(ts)
    if cnt >= 64:
        # many texts: the arrays are views of ONE allocation and the pointer tables come out of numpy -- a ctypes pointer per
        # text costs more than the library needs to build a small text (k_small_sa_batch: 0.04-1.6 us per text)
        sizes = np.fromiter((t.size for t in ts), dtype=np.int64, count=cnt)
        offs = np.zeros(cnt + 1, dtype=np.int64)
        np.cumsum(sizes + 1, out=offs[1:])
        buf = np.empty(int(offs[-1]), dtype=np.uint32)
        outs = [buf[a:b] for a, b in zip(offs[:-1].tolist(), offs[1:].tolist())]
        tp = np.fromiter((t.__array_interface__["data"][0] for t in ts), dtype=np.uint64, count=cnt)
        sp = (np.uint64(buf.ctypes.data) + (offs[:-1] * 4).astype(np.uint64)).astype(np.uint64)
        nn = sizes.astype(np.int32)
        dd = np.asarray(devices, dtype=np.int32) if devices is not None else None
        st = np.zeros(cnt, dtype=np.int32)
        rc = lib().sa_amd_saca_batch(tp.ctypes.data, sp.ctypes.data, nn.ctypes.data, dd.ctypes.data if dd is not None else None, cnt,
                                     st.ctypes.data)
        _check(rc)
        return outs
    outs = [np.empty(t.size + 1, dtype=np.uint32) for t in ts]
    T = (ctypes.c_void_p * cnt)(*[t.ctypes.data for t in ts])
    S = (ctypes.c_void_p * cnt)(*[o.ctypes.data for o in outs])
    N = (ctypes.c_int32 * cnt)(*[t.size for t in ts])
    D = (ctypes.c_int32 * cnt)(*devices) if devices is not None else None
    st = (ctypes.c_int32 * cnt)()
    rc = lib().sa_amd_saca_batch(T, S, N, D, cnt, st)
    _check(rc)
    return outs


def last_host_timing() -> dict:
    """wall-clock phases (ms) of this thread's most recent host-pointer build (sa_amd_last_host_timing)"""
    v = (ctypes.c_double * 9)()
    lib().sa_amd_last_host_timing(v, 9)
    return {"acquire": v[0], "h2d": v[1], "build": v[2], "d2h": v[3], "release": v[4], "total": v[5], "staged_threads": int(v[6]),
            "early_fraction": v[7], "workspace_bytes_in_host_memory": int(v[8])}


def last_stats() -> dict:
    """statistics of the most recent build issued by this thread"""
    st = Stats()
    lib().sa_amd_last_stats(ctypes.byref(st))
    return st.as_dict()


BUCKET_TABLE_LEN = 256 * 257 + 1        # reference src/sa.rs:95


def bucket_table(s, sa: np.ndarray | None = None) -> np.ndarray:
    """the table `enable_buckets` builds (reference src/sa.rs:89-119), computed on the GPU the way the reference computes
    it: bigram counts of the TEXT + prefix sum (src/sa.rs:96-116).  `sa` is not needed (and not uploaded); it is accepted for
    callers of the earlier form and only its length is checked"""
    t = _as_u8(s)
    if sa is not None:
        assert np.asarray(sa).size == t.size + 1
    bkt = np.empty(BUCKET_TABLE_LEN, dtype=np.uint32)
    _check(lib().sa_amd_bucket_table(t.ctypes.data, t.size, None, bkt.ctypes.data))
    return bkt


def check_integrity(s, sa: np.ndarray) -> bool:
    """`check_integrity` (reference src/sa.rs:72-84) on the GPU; raises IndexError where the
    reference panics (an entry beyond the text)"""
    t = _as_u8(s)
    a = np.ascontiguousarray(sa, dtype=np.uint32)
    rc = lib().sa_amd_check_integrity(t.ctypes.data, t.size, a.ctypes.data, a.size)
    if rc == -6:
        raise IndexError("suffix offset out of range (the reference panics here, src/sa.rs:77-78)")
    if rc < 0:
        _check(rc)
    return rc == 1


def pack(sa: np.ndarray) -> bytes:
    """`PackedSuffixArray::from_sa(..).dump_bytes()` -- reference src/packed_sa.rs:17-53, :99-106 (bit packing on the GPU)"""
    a = np.ascontiguousarray(sa, dtype=np.uint32)
    cap = int(lib().sa_amd_pack_bound(a.size))
    out = np.empty(cap, dtype=np.uint8)
    n_out = ctypes.c_int64()
    _check(lib().sa_amd_pack(a.ctypes.data, a.size, out.ctypes.data, cap, ctypes.byref(n_out)))
    return out[:n_out.value].tobytes()


def unpack(blob: bytes) -> np.ndarray:
    """`PackedSuffixArray::load_bytes(..).into_sa()` -- reference src/packed_sa.rs:55-88, :117-124;
    ValueError where the reference returns an InvalidData error"""
    b = np.frombuffer(blob, dtype=np.uint8)
    if b.size < 16:
        raise ValueError("packed suffix array: truncated header")
    length = int(np.frombuffer(blob[4:8], dtype="<u4")[0])
    out = np.empty(max(length, 1), dtype=np.uint32)
    got = ctypes.c_int64()
    rc = lib().sa_amd_unpack(b.ctypes.data, b.size, out.ctypes.data, out.size, ctypes.byref(got))
    if rc == -1:
        raise ValueError("packed suffix array: invalid data")
    _check(rc)
    return out[:got.value]


def _lcp_rc(rc: int) -> None:
    if rc == -6:
        raise IndexError("suffix offset out of range")
    _check(rc)


def lcp(s, sa: np.ndarray) -> np.ndarray:
    """LCP array of the text and its suffix array (an extension the reference lacks: its README's TODO "construct enhanced
    suffix array"), computed on the GPU: uint32, ``len(s) + 1`` entries aligned with ``sa`` (``sa[0] == len(s)``);
    ``lcp[0] == 0`` and ``lcp[i]`` is the longest common prefix of the suffixes at ``sa[i-1]`` and ``sa[i]``.  ``sa`` must
    be the suffix array of ``s`` (not proved here; ``check_integrity`` does that): IndexError for an entry > len(s)."""
    t = _as_u8(s)
    a = np.ascontiguousarray(sa, dtype=np.uint32)
    assert a.size == t.size + 1
    out = np.empty(t.size + 1, dtype=np.uint32)
    _lcp_rc(lib().sa_amd_lcp(t.ctypes.data, t.size, a.ctypes.data, out.ctypes.data))
    return out


def saca_lcp(s):
    """-> (sa, lcp): the suffix array (layout of ``saca``) and its LCP array in one device round trip"""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = np.empty(t.size + 1, dtype=np.uint32)
    out = np.empty(t.size + 1, dtype=np.uint32)
    _check(lib().sa_amd_saca_u8_lcp(t.ctypes.data, a.ctypes.data, t.size, out.ctypes.data))
    return a, out


def last_lcp_stats() -> dict:
    """irreducible / compared_bytes / long_pairs / readbacks of this thread's most recent LCP build"""
    st = LcpStats()
    lib().sa_amd_last_lcp_stats(ctypes.byref(st))
    return st.as_dict()


def lcp_set_compare_cap(nbytes: int) -> int:
    """route switch for this thread's later LCP builds (never changes a result): bytes one lane compares before a pair goes to
    the long-compare path, clamped to 0 .. 2**20; negative restores the default (64).  Returns the previous value."""
    return int(lib().sa_amd_lcp_set_compare_cap(int(nbytes)))


def last_search_stats() -> dict:
    """sa_amd_search_stats of this thread's most recent DeviceIndex.search: route 1 (LCP route, enable_lcp) with the compared
    bytes, tree steps and steps decided from the table; route 0 (plain binary search) with those counters at -1"""
    st = SearchStats()
    lib().sa_amd_last_search_stats(ctypes.byref(st))
    return st.as_dict()


def lcp_work_bytes(n: int) -> int:
    return int(lib().sa_amd_lcp_work_bytes(n))


def lcp_device_ptr(text_ptr: int, sa_ptr: int, n: int, lcp_ptr: int, work_ptr: int, work_bytes: int, stream: int = 0) -> None:
    """Device-resident LCP build (raw device pointers, e.g. torch ``tensor.data_ptr()``); blocks until done."""
    _lcp_rc(lib().sa_amd_lcp_device(text_ptr, sa_ptr, n, lcp_ptr, work_ptr, work_bytes, stream))


def _bwt_rc(rc: int) -> None:
    if rc == -6:
        raise IndexError("suffix offset out of range")
    if rc == -1:
        raise ValueError("invalid argument: not a suffix array of this layout / not a Burrows-Wheeler transform")
    _check(rc)


def bwt(s, sa: Optional[np.ndarray] = None):
    """-> (b, primary): the Burrows-Wheeler transform of ``s`` on the GPU (the layout of libdivsufsort's ``divbwt`` as
    restated in include/suffix_array_amd.h).  With ``sa`` in the layout of ``saca`` (``sa[0] == len(s)``), ``primary`` is the
    slot with ``sa[primary] == 0`` and ``b`` (uint8, ``len(s)`` bytes) is ``s[sa[k] - 1]`` for ``k < primary`` and
    ``s[sa[k + 1] - 1]`` from there on.  ``sa=None``: the array is built on the device and never downloaded.
    IndexError for an entry > len(s); ValueError when ``sa[0] != len(s)`` or not exactly one entry is 0."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = None
    if sa is not None:
        a = np.ascontiguousarray(sa, dtype=np.uint32)
        assert a.size == t.size + 1
    out = np.empty(t.size, dtype=np.uint8)
    primary = ctypes.c_int32(0)
    _bwt_rc(lib().sa_amd_bwt(t.ctypes.data, t.size, None if a is None else a.ctypes.data, out.ctypes.data, ctypes.byref(primary)))
    return out, int(primary.value)


def unbwt(b, primary: int) -> np.ndarray:
    """the text whose transform is ``(b, primary)`` (see ``bwt``), on the GPU; ValueError when ``primary`` is outside
    1 .. len(b) (0 for the empty string) or the pair is not the transform of any text"""
    t = _as_u8(b)
    assert t.size <= MAX_LENGTH
    if not -2**31 <= int(primary) < 2**31:
        raise ValueError("primary index out of range")
    out = np.empty(t.size, dtype=np.uint8)
    _bwt_rc(lib().sa_amd_unbwt(t.ctypes.data, t.size, int(primary), out.ctypes.data))
    return out


def last_unbwt_stats() -> dict:
    """walkers / steps / longest_walk / splitter_spacing / walk_launches / restarts / readbacks of this thread's most recent
    inverse transform"""
    st = UnbwtStats()
    lib().sa_amd_last_unbwt_stats(ctypes.byref(st))
    return st.as_dict()


def unbwt_set_walk_limits(cap_steps: int = -1, max_launches: int = -1) -> None:
    """route switch for this thread's later inverse transforms (never changes a result): steps one lane walks per launch, and
    walk launches after which an attempt restarts with denser splitters; a negative value restores that default"""
    lib().sa_amd_unbwt_set_walk_limits(int(cap_steps), int(max_launches))


def unbwt_set_splitter_spacing(spacing: int = -1) -> int:
    """route switch for this thread's later inverse transforms (never changes a result): the splitter spacing S of the first
    attempt, rounded down to a power of two in 4 .. 65536; negative restores the default (256).  Returns the previous value."""
    return int(lib().sa_amd_unbwt_set_splitter_spacing(int(spacing)))


def bwt_work_bytes(n: int) -> int:
    return int(lib().sa_amd_bwt_work_bytes(n))


def unbwt_work_bytes(n: int) -> int:
    return int(lib().sa_amd_unbwt_work_bytes(n))


def bwt_device_ptr(text_ptr: int, sa_ptr: int, n: int, bwt_ptr: int, work_ptr: int, work_bytes: int, stream: int = 0) -> int:
    """Device-resident forward transform (raw device pointers, e.g. torch ``tensor.data_ptr()``); blocks until done and
    returns the primary index."""
    primary = ctypes.c_int32(0)
    _bwt_rc(lib().sa_amd_bwt_device(text_ptr, sa_ptr, n, bwt_ptr, ctypes.byref(primary), work_ptr, work_bytes, stream))
    return int(primary.value)


def unbwt_device_ptr(bwt_ptr: int, n: int, primary: int, text_ptr: int, work_ptr: int, work_bytes: int, stream: int = 0) -> None:
    """Device-resident inverse transform (raw device pointers); blocks until done."""
    _bwt_rc(lib().sa_amd_unbwt_device(bwt_ptr, n, int(primary), text_ptr, work_ptr, work_bytes, stream))


def _repeat_min_len(min_len) -> int:
    k = int(min_len)
    if k < 1:
        raise ValueError("min_len must be at least 1")
    return min(k, 2**31 - 1)            # (no repeat is longer than MAX_LENGTH - 1: a larger threshold gives the same, empty, answer)


def repeat_spans_bound(n: int, min_len: int) -> int:
    """no text of ``n`` bytes has more spans of threshold ``min_len`` than this: ``(n + 1) // (min_len + 1)``"""
    return int(lib().sa_amd_repeat_spans_bound(int(n), _repeat_min_len(min_len)))


def repeat_lengths(s, sa: Optional[np.ndarray] = None) -> np.ndarray:
    """Longest-repeat array of ``s`` on the GPU: uint32, ``len(s)`` entries in text order; ``lr[p]`` is the length of the
    longest substring starting at ``p`` that also starts at some other position.  With the LCP array of ``lcp``,
    ``lr[sa[i]] == max(lcp[i], lcp[i + 1])``.  ``sa=None``: the array is built on the device and never downloaded; else it
    must be the suffix array of ``s`` in the layout of ``saca`` (IndexError for an entry > len(s), ValueError when
    ``sa[0] != len(s)``)."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = None
    if sa is not None:
        a = np.ascontiguousarray(sa, dtype=np.uint32)
        assert a.size == t.size + 1
    out = np.empty(t.size, dtype=np.uint32)
    _bwt_rc(lib().sa_amd_repeat_lengths(t.ctypes.data, t.size, None if a is None else a.ctypes.data, out.ctypes.data))
    return out


def repeat_spans(s, min_len: int, keep_first: bool = False, sa: Optional[np.ndarray] = None) -> np.ndarray:
    """Byte ranges of ``s`` that are copies, on the GPU: a ``(count, 2)`` uint32 array of ``[start, end)`` rows, ascending,
    disjoint and not adjacent.  ``keep_first=False``: every byte inside some occurrence of a substring of at least
    ``min_len`` bytes that occurs at least twice (first occurrences included).  ``keep_first=True``: the union of the windows
    ``s[p : p + min_len]`` that equal a window starting earlier -- the first copy of everything survives, which is what a
    deduplicator removes.  ``sa`` as for ``repeat_lengths``; only the spans come back from the device."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    k = _repeat_min_len(min_len)
    a = None
    if sa is not None:
        a = np.ascontiguousarray(sa, dtype=np.uint32)
        assert a.size == t.size + 1
    cap = (t.size + 1) // (k + 1)
    out = np.empty((cap, 2), dtype=np.uint32)
    count = ctypes.c_int64(0)
    _bwt_rc(lib().sa_amd_repeat_spans(t.ctypes.data, t.size, None if a is None else a.ctypes.data, k,
                                      REPEATS_KEEP_FIRST if keep_first else REPEATS_ALL, out.ctypes.data, cap, ctypes.byref(count)))
    return out[:min(int(count.value), cap)].copy()


def last_repeat_stats() -> dict:
    """longest / longest_pos / lcp_sum / distinct_substrings / spans / covered_bytes / flagged / readbacks of this thread's
    most recent repeat call (the span fields read 0 after ``repeat_lengths``)"""
    st = RepeatStats()
    lib().sa_amd_last_repeat_stats(ctypes.byref(st))
    return st.as_dict()


def repeats_work_bytes(n: int) -> int:
    return int(lib().sa_amd_repeats_work_bytes(n))


def repeat_lengths_device_ptr(text_ptr: int, sa_ptr: int, n: int, lr_ptr: int, work_ptr: int, work_bytes: int, stream: int = 0) -> None:
    """Device-resident longest-repeat array (raw device pointers, e.g. torch ``tensor.data_ptr()``); blocks until done."""
    _bwt_rc(lib().sa_amd_repeat_lengths_device(text_ptr, sa_ptr, n, lr_ptr, work_ptr, work_bytes, stream))


def repeat_spans_device_ptr(text_ptr: int, sa_ptr: int, n: int, min_len: int, mode: int, spans_ptr: int, capacity: int,
                            work_ptr: int, work_bytes: int, stream: int = 0) -> int:
    """Device-resident spans (raw device pointers; ``spans_ptr``: ``2 * capacity`` uint32); blocks until done and returns the
    number of all spans, of which the first ``capacity`` have been written."""
    count = ctypes.c_int64(0)
    _bwt_rc(lib().sa_amd_repeat_spans_device(text_ptr, sa_ptr, n, int(min_len), int(mode), spans_ptr, int(capacity),
                                             ctypes.byref(count), work_ptr, work_bytes, stream))
    return int(count.value)


def _sa_arg(t, sa):
    if sa is None:
        return None
    a = np.ascontiguousarray(sa, dtype=np.uint32)
    assert a.size == t.size + 1
    return a


def lpf(s, sa: Optional[np.ndarray] = None):
    """Longest-previous-factor array of ``s`` on the GPU, with a source for every position: ``(LPF, SRC)``, two uint32 arrays of
    ``len(s)`` entries in text order.  ``LPF[p]`` is the length of the longest prefix of ``s[p:]`` that also starts at some
    ``q < p`` (the copy may overlap ``p``); ``SRC[p]`` is such a ``q`` -- of the two suffix-array neighbours with a smaller
    position the one with the longer match, the left one on a tie -- or ``LZ_LITERAL`` where ``LPF[p] == 0``.  ``sa`` as for
    ``repeat_lengths``."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = _sa_arg(t, sa)
    out = np.empty((2, t.size), dtype=np.uint32)
    _bwt_rc(lib().sa_amd_lpf(t.ctypes.data, t.size, None if a is None else a.ctypes.data, out[0].ctypes.data, out[1].ctypes.data))
    return out[0], out[1]


def lz77(s, sa: Optional[np.ndarray] = None) -> np.ndarray:
    """Greedy LZ77 parse of ``s`` on the GPU: a ``(z, 2)`` uint32 array of ``(source, length)`` rows.  Phrase starts are
    ``s_0 = 0``, ``s_{k+1} = s_k + max(1, LPF[s_k])``; row ``k`` is ``(SRC[s_k], max(1, LPF[s_k]))``, a literal byte
    ``(LZ_LITERAL, 1)``.  The lengths sum to ``len(s)``; ``lz77_decode`` takes them together with the literal bytes
    (``lz77_literals``).  Only the phrases come back from the device."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = _sa_arg(t, sa)
    cap = min(t.size, max(1 << 16, t.size // 8))        # (a second call when there are more phrases than that)
    while True:
        out = np.empty((cap, 2), dtype=np.uint32)
        count = ctypes.c_int64(0)
        _bwt_rc(lib().sa_amd_lz77(t.ctypes.data, t.size, None if a is None else a.ctypes.data, out.ctypes.data, cap, ctypes.byref(count)))
        if count.value <= cap:
            return out[:int(count.value)].copy()
        cap = int(count.value)


def lz77_literals(s, phrases) -> bytes:
    """the bytes of the literal phrases of ``phrases`` (a parse of ``s``), in phrase order: what a parse needs besides its
    ``(source, length)`` rows to be decoded"""
    t = _as_u8(s)
    ph = np.asarray(phrases, dtype=np.int64).reshape(-1, 2)
    starts = np.cumsum(ph[:, 1]) - ph[:, 1]
    return t[starts[ph[:, 0] == LZ_LITERAL]].tobytes()


def lz77_decode(phrases, literals) -> bytes:
    """Host helper, not a GPU path: the text of a parse.  ``phrases`` as ``lz77`` returns them, ``literals`` the bytes of the
    literal phrases in order (``lz77_literals``): a ``(LZ_LITERAL, 1)`` row does not carry its byte.  Copies go byte by byte,
    because a source may overlap its own phrase."""
    lit = bytes(_as_u8(literals))
    out = bytearray()
    k = 0
    for src, ln in np.asarray(phrases, dtype=np.int64).reshape(-1, 2).tolist():
        if src == LZ_LITERAL:
            out.append(lit[k])
            k += 1
        else:
            for j in range(ln):
                out.append(out[src + j])
    return bytes(out)


def last_lz_stats() -> dict:
    """phrases / literals / longest / longest_pos / unresolved / hierarchy_steps / hierarchy_max / walkers / walk_steps /
    walk_launches / restarts / splitter_spacing / readbacks of this thread's most recent ``lpf`` / ``lz77`` call (the phrase and
    walk fields read 0 after ``lpf``); ``last_lcp_stats`` holds the compares of both value passes together"""
    st = LzStats()
    lib().sa_amd_last_lz_stats(ctypes.byref(st))
    return st.as_dict()


def lz_work_bytes(n: int) -> int:
    return int(lib().sa_amd_lz_work_bytes(n))


def lpf_device_ptr(text_ptr: int, sa_ptr: int, n: int, lpf_ptr: int, src_ptr: int, work_ptr: int, work_bytes: int, stream: int = 0) -> None:
    """Device-resident LPF and SRC (raw device pointers, either output may be 0); blocks until done."""
    _bwt_rc(lib().sa_amd_lpf_device(text_ptr, sa_ptr, n, lpf_ptr or None, src_ptr or None, work_ptr, work_bytes, stream))


def lz77_device_ptr(text_ptr: int, sa_ptr: int, n: int, phrases_ptr: int, capacity: int, work_ptr: int, work_bytes: int,
                    stream: int = 0) -> int:
    """Device-resident parse (raw device pointers; ``phrases_ptr``: ``2 * capacity`` uint32); blocks until done and returns the
    number of all phrases, of which the first ``capacity`` have been written."""
    count = ctypes.c_int64(0)
    _bwt_rc(lib().sa_amd_lz77_device(text_ptr, sa_ptr, n, phrases_ptr or None, int(capacity), ctypes.byref(count), work_ptr, work_bytes,
                                     stream))
    return int(count.value)


def _substr_rows(n: int, query: SubstrQuery, positions: bool, call):
    """the two-call protocol of the substrings routes: ``call(query, rows_ptr, pos_ptr, capacity, total)`` -> return code"""
    bound = max(n - 1, 0)
    cap = min(bound, int(query.k)) if query.order != SUBSTR_ALL and query.k >= 1 else min(bound, max(1 << 16, n // 8))
    while True:
        rows = np.empty((cap, 4), dtype=np.uint32)
        pos = np.empty(cap, dtype=np.uint32) if positions else None
        total = ctypes.c_int64(0)
        _bwt_rc(call(ctypes.byref(query), rows.ctypes.data if cap else None, pos.ctypes.data if positions and cap else None, cap,
                     ctypes.byref(total)))
        if total.value <= cap:
            r = rows[:int(total.value)].copy()
            return (r, pos[:int(total.value)].copy()) if positions else r
        cap = int(total.value)


def repeated_substrings(s, min_len: int = 1, max_len: int = 0, min_count: int = 2, order: int = SUBSTR_ALL, k: int = 0,
                        sa: Optional[np.ndarray] = None, positions: bool = False):
    """The substrings of ``s`` that occur at least twice, as the internal nodes of its suffix tree, on the GPU: a ``(rows, 4)``
    uint32 array of ``(lo, count, depth, parent)``.  The node's substring has ``depth`` bytes, occurs exactly ``count`` times,
    at ``SA[lo : lo + count]``, and so does every prefix of it longer than ``parent``.  A node is selected when
    ``depth >= min_len``, ``max_len == 0 or parent < max_len`` and ``count >= min_count``; its effective length is ``depth``,
    cut to ``max_len`` when that is not 0.  ``SUBSTR_ALL`` returns every selected node in suffix-array order; ``SUBSTR_BY_COUNT``,
    ``SUBSTR_BY_LENGTH`` and ``SUBSTR_BY_COVER`` (count times length) return the best ``k`` by that key, ties in suffix-array
    order.  ``positions=True`` adds ``pos`` with ``pos[r] = SA[lo_r]``: ``s[pos[r] : pos[r] + depth_r]`` is row ``r``'s
    substring.  ``sa`` as for ``repeat_lengths``; neither the suffix array nor the LCP array comes back from the device."""
    t = _as_u8(s)
    assert t.size <= MAX_LENGTH
    a = _sa_arg(t, sa)
    q = SubstrQuery(int(min_len), int(max_len), int(min_count), int(order), int(k))
    return _substr_rows(t.size, q, positions, lambda qp, rp, pp, cap, tot: lib().sa_amd_substrings(
        t.ctypes.data, t.size, None if a is None else a.ctypes.data, qp, rp, pp, cap, tot))


def last_substr_stats() -> dict:
    """nodes / selected / distinct_all / distinct_selected / unresolved / far_steps / far_max / sorted / select_passes / readbacks
    of this thread's most recent ``repeated_substrings`` call; ``last_lcp_stats`` holds the LCP build inside it"""
    st = SubstrStats()
    lib().sa_amd_last_substr_stats(ctypes.byref(st))
    return st.as_dict()


def substrings_work_bytes(n: int) -> int:
    return int(lib().sa_amd_substrings_work_bytes(n))


def substrings_bound(n: int) -> int:
    """the most rows any ``repeated_substrings`` query of an ``n``-byte text can have: ``max(n - 1, 0)``"""
    return int(lib().sa_amd_substrings_bound(n))


def last_doc_substr_stats() -> dict:
    """nodes / selected / distinct_selected / df_sum / max_df / pairs / rmq_far / rmq_steps / rmq_max / sorted / select_passes /
    readbacks of this thread's most recent ``doc_substrings`` call; ``last_lcp_stats`` holds the LCP build inside it"""
    st = DocSubstrStats()
    lib().sa_amd_last_doc_substr_stats(ctypes.byref(st))
    return st.as_dict()


def doc_substrings_work_bytes(n: int) -> int:
    return int(lib().sa_amd_doc_substrings_work_bytes(n))


def substrings_device_ptr(text_ptr: int, sa_ptr: int, n: int, query: SubstrQuery, rows_ptr: int, pos_ptr: int, capacity: int,
                          work_ptr: int, work_bytes: int, stream: int = 0) -> int:
    """Device-resident rows (raw device pointers; ``rows_ptr``: ``4 * capacity`` uint32, ``pos_ptr``: ``capacity`` uint32 or 0);
    blocks until done and returns the number of all rows of the query, of which the first ``capacity`` have been written."""
    total = ctypes.c_int64(0)
    _bwt_rc(lib().sa_amd_substrings_device(text_ptr, sa_ptr, n, ctypes.byref(query), rows_ptr or None, pos_ptr or None, int(capacity),
                                           ctypes.byref(total), work_ptr, work_bytes, stream))
    return int(total.value)


def last_match_stats() -> dict:
    """positions / matched / longest / longest_pos / ml_sum / long_positions / compared_bytes / steps / spans / covered_bytes /
    flagged / route_long / readbacks / group_lanes / group_cap / tile of this thread's most recent ``match_stats`` /
    ``match_spans`` call (the span fields read 0 after ``match_stats``)"""
    st = MatchStats()
    lib().sa_amd_last_match_stats(ctypes.byref(st))
    return st.as_dict()


def match_work_bytes(m: int) -> int:
    return int(lib().sa_amd_match_work_bytes(m))


def match_set_group_cap(nbytes: int) -> int:
    """Route switch of this thread's later match calls (never changes a result): window bytes a lane group compares before the
    position goes to the one-wave-per-position path, 0 .. 1 048 576 (0: every position; above 4096 acts as 4096); negative
    restores the default (64).  Returns the previous value."""
    return int(lib().sa_amd_match_set_group_cap(int(nbytes)))


def match_set_group_lanes(lanes: int) -> int:
    """The same kind of switch for the lanes that serve one query position on the group path: 4, 8 or 16 (default 8; negative
    restores it).  Returns the previous value."""
    return int(lib().sa_amd_match_set_group_lanes(int(lanes)))


def _index_handle(index):
    return index._h if isinstance(index, DeviceIndex) else index


def match_stats_device_ptr(index, query_ptr: int, m: int, max_len: int, ml_ptr: int, pos_ptr: int, work_ptr: int, work_bytes: int,
                           stream: int = 0) -> None:
    """Device-resident matching statistics of ``m`` query bytes against ``index`` (a ``DeviceIndex``; raw device pointers on its
    device, either output may be 0); blocks until done."""
    _check(lib().sa_amd_index_match_stats_device(_index_handle(index), query_ptr or None, int(m), int(max_len), ml_ptr or None,
                                                 pos_ptr or None, work_ptr, work_bytes, stream))


def match_spans_device_ptr(index, query_ptr: int, m: int, min_len: int, spans_ptr: int, capacity: int, work_ptr: int, work_bytes: int,
                           stream: int = 0) -> int:
    """Device-resident shared spans (``spans_ptr``: ``2 * capacity`` uint32); blocks until done and returns the number of all
    spans, of which the first ``capacity`` have been written."""
    count = ctypes.c_int64(0)
    _check(lib().sa_amd_index_match_spans_device(_index_handle(index), query_ptr or None, int(m), int(min_len), spans_ptr or None,
                                                 int(capacity), ctypes.byref(count), work_ptr, work_bytes, stream))
    return int(count.value)


def last_docs_stats() -> dict:
    """patterns / occ_sum / units / df_sum / slots_scanned / chunk / readbacks / listed of this thread's most recent
    ``doc_search`` / ``doc_list`` call"""
    st = DocsStats()
    lib().sa_amd_last_docs_stats(ctypes.byref(st))
    return st.as_dict()


def docs_work_bytes(n: int) -> int:
    """device scratch ``set_documents`` takes from the pool for a text of ``n`` bytes"""
    return int(lib().sa_amd_docs_work_bytes(n))


def last_doc_repeat_stats() -> dict:
    """members / flagged / spans / covered_bytes / docs_touched / readbacks of this thread's most recent ``doc_repeat_spans``
    call (``docs_touched`` is -1 when the call did not ask for ``doc_bytes``)"""
    st = DocRepeatStats()
    lib().sa_amd_last_doc_repeat_stats(ctypes.byref(st))
    return st.as_dict()


def doc_repeats_work_bytes(n: int, ndocs: int) -> int:
    """device scratch ``doc_repeat_spans`` takes from the pool for a text of ``n`` bytes in ``ndocs`` documents"""
    return int(lib().sa_amd_doc_repeats_work_bytes(int(n), int(ndocs)))


def docs_set_chunk(slots: int) -> int:
    """Route switch of this thread's later ``doc_search`` / ``doc_list`` calls (never changes a result): slots of a match range
    one wave scans, ``DOC_CHUNK_MIN`` .. ``DOC_CHUNK_MAX``; negative restores ``DOC_CHUNK_DEFAULT``.  Returns the previous value."""
    return int(lib().sa_amd_docs_set_chunk(int(slots)))


def last_doc_tf_stats() -> dict:
    """patterns / occ_sum / df_sum / tf_sum / table_loads / topk_entries / pieces / rounds / k / piece / chunk / readbacks of this
    thread's most recent ``doc_tf`` / ``doc_topk`` call"""
    st = DocTfStats()
    lib().sa_amd_last_doc_tf_stats(ctypes.byref(st))
    return st.as_dict()


def docs_set_topk_piece(entries: int) -> int:
    """Route switch of this thread's later ``doc_topk`` calls (never changes a result): keys of a piece of the reduction, rounded
    down to a power of two in ``DOC_TOPK_PIECE_MIN`` .. ``DOC_TOPK_PIECE_MAX``; negative restores ``DOC_TOPK_PIECE_DEFAULT``.
    Returns the previous value."""
    return int(lib().sa_amd_docs_set_topk_piece(int(entries)))


def last_ngram_stats() -> dict:
    """patterns / range_searches / compared_bytes / stream_slots / search_slots / stream_queries / search_queries / empty_queries /
    entries / stream_cap / readbacks / backoff / passes of this thread's most recent ``next_bytes`` / ``infgram`` call"""
    st = NgramStats()
    lib().sa_amd_last_ngram_stats(ctypes.byref(st))
    return st.as_dict()


def ngram_set_stream_cap(slots: int) -> int:
    """Route switch of this thread's later ``next_bytes`` / ``infgram`` calls (never changes a result): match ranges of at most
    ``slots`` slots are streamed, longer ones have their run starts searched; 0 searches every range, a huge value streams every
    range, negative restores ``NGRAM_STREAM_CAP_DEFAULT``.  Returns the previous value."""
    return int(lib().sa_amd_ngram_set_stream_cap(max(-1, min(int(slots), 2**31 - 1))))


def last_score_stats() -> dict:
    """positions / documents / group_searches / long_searches / range_searches (their sum) / next_lookups / compared_bytes /
    long_positions / zero_positions / group_cap / readbacks of this thread's most recent ``infgram_score`` call"""
    st = ScoreStats()
    lib().sa_amd_last_score_stats(ctypes.byref(st))
    return st.as_dict()


def score_set_group_cap(nbytes: int) -> int:
    """Route switch of this thread's later ``infgram_score`` calls (never changes a result): context bytes a lane group probes
    before the position goes to the one-wave-per-position path, 0 .. 1 048 576 (0: every position with a context; above 4096
    acts as 4096); negative restores ``SCORE_GROUP_CAP_DEFAULT``.  Returns the previous value.  The same switch applies to
    ``TokenIndex.infgram_score``, where it counts context tokens."""
    return int(lib().sa_amd_score_set_group_cap(max(-1, min(int(nbytes), 2**31 - 1))))


def score_work_bytes(m: int, ndocs: int = 1) -> int:
    return int(lib().sa_amd_score_work_bytes(int(m), int(ndocs)))


def _score_offsets(doc_offsets):
    if doc_offsets is None:
        return None, 0
    off = np.ascontiguousarray(doc_offsets)
    if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
        raise SuffixArrayError(-1, "infgram_score: doc_offsets are ndocs + 1 integers")
    off = off.astype(np.int64)
    return off, int(off.size - 1)


def infgram_score_device_ptr(index, query_ptr: int, m: int, min_count: int, max_len: int, s_ptr: int, lo_ptr: int, hi_ptr: int,
                             at_end_ptr: int, nlo_ptr: int, nhi_ptr: int, work_ptr: int, work_bytes: int, doc_offsets=None,
                             stream: int = 0) -> None:
    """Device-resident ``infgram_score`` of ``m`` query bytes against ``index`` (a ``DeviceIndex``; raw device pointers on its
    device, any output may be 0; ``doc_offsets`` stays a host array); blocks until done."""
    off, ndocs = _score_offsets(doc_offsets)
    _check(lib().sa_amd_index_infgram_score_device(_index_handle(index), query_ptr or None, int(m), off.ctypes.data if off is not None else None,
                                                   ndocs, int(min_count), int(max_len), s_ptr or None, lo_ptr or None, hi_ptr or None,
                                                   at_end_ptr or None, nlo_ptr or None, nhi_ptr or None, work_ptr or None, int(work_bytes), stream))


def doc_of_device_ptr(index, pos_ptr: int, count: int, doc_ptr: int, stream: int = 0) -> None:
    """Device-resident ``doc_of``: ``count`` uint32 positions at ``pos_ptr`` -> their documents at ``doc_ptr`` (raw device pointers
    on the index's device, 4-byte aligned); needs no scratch; blocks until done."""
    _check(lib().sa_amd_index_doc_of_device(_index_handle(index), pos_ptr or None, int(count), doc_ptr or None, stream))


def _pattern_batch(patterns):
    pats = [bytes(p) for p in patterns]
    off = np.zeros(len(pats) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in pats])
    data = np.frombuffer(b"".join(pats), dtype=np.uint8) if off[-1] else np.zeros(1, dtype=np.uint8)
    return data, off, len(pats)


def _is_pattern(x) -> bool:
    return isinstance(x, (bytes, bytearray, memoryview, str)) or (isinstance(x, np.ndarray) and x.dtype == np.uint8)


def _as_pattern(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


def _query_batch(queries, is_pattern=_is_pattern, as_pattern=_as_pattern, batch=_pattern_batch):
    """queries -> (pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries) in the layout of
    sa_amd_index_doc_match.  A query is a sequence of clauses; a clause is one pattern, a sequence of patterns (any of them), or
    ``Not(...)`` of either.  The token indexes pass their own idea of a pattern and their own batch."""
    pats, clause_off, flags, query_off = [], [0], [], [0]
    for query in queries:
        if is_pattern(query) or isinstance(query, Not):
            raise TypeError("a query is a sequence of clauses: wrap a single clause in a list")
        for clause in query:
            neg = isinstance(clause, Not)
            body = clause.clause if neg else clause
            pats += [as_pattern(body)] if is_pattern(body) else [as_pattern(p) for p in body]
            clause_off.append(len(pats))
            flags.append(1 if neg else 0)
        query_off.append(len(flags))
    data, off, cnt = batch(pats)
    cfl = np.array(flags + [0], dtype=np.uint8)                       # (never a zero-sized buffer)
    return (data, off, cnt, np.array(clause_off, dtype=np.int32), cfl, len(flags), np.array(query_off, dtype=np.int32), len(query_off) - 1)


def last_doc_match_stats() -> dict:
    """patterns / clauses / queries / occ_sum / units / marks / bitmap_words / slabs / df_sum / budget / chunk / readbacks /
    listed of this thread's most recent ``doc_match`` / ``doc_match_list`` call"""
    st = DocMatchStats()
    lib().sa_amd_last_doc_match_stats(ctypes.byref(st))
    return st.as_dict()


def doc_match_set_budget(nbytes: int) -> int:
    """Route switch of this thread's later ``doc_match`` / ``doc_match_list`` calls (never changes a result): the bytes of
    clause bitmaps one slab of queries may hold, 4 KiB .. 2^40; negative restores the default of 256 MiB.  Returns the previous
    value."""
    return int(lib().sa_amd_doc_match_set_budget(int(nbytes)))


def _ngram_query(next_fn, infgram_fn, handle, batch, sym_dtype, cap: int, backoff: bool, min_count: int, max_len: int):
    """the continuation query of either index (``next_fn`` / ``infgram_fn`` of its ABI) over an uploaded ``batch`` of patterns ->
    ``(suffix_len, lo, hi, at_end, list_off, symbols, counts)``; a listing longer than ``cap`` entries is asked for again with
    the capacity the first call reported"""
    data, off, cnt = batch
    slen, lo, hi = (np.zeros(cnt, dtype=np.uint32) for _ in range(3))
    ae = np.zeros(cnt, dtype=np.uint8)
    loff = np.zeros(cnt + 1, dtype=np.int64)
    total = ctypes.c_int64(0)
    while True:
        syms = np.empty(max(cap, 1), dtype=sym_dtype)
        c = np.empty(max(cap, 1), dtype=np.uint32)
        out = (lo.ctypes.data, hi.ctypes.data, ae.ctypes.data, loff.ctypes.data, syms.ctypes.data, c.ctypes.data, cap, ctypes.byref(total))
        if backoff:
            _check(infgram_fn(handle, data.ctypes.data, off.ctypes.data, cnt, int(min_count), int(max_len), slen.ctypes.data, *out))
        else:
            _check(next_fn(handle, data.ctypes.data, off.ctypes.data, cnt, *out))
        if total.value <= cap:
            m = int(total.value)
            return slen, lo, hi, ae, loff, syms[:m].copy(), c[:m].copy()
        cap = int(total.value)


class DeviceIndex:
    """Text + suffix array resident in HBM (sa_amd_index of include/suffix_array_amd.h): batched
    `contains` / `search_all` / `search_lcp` (reference src/sa.rs:164-253), bucket table, integrity check.
    `sa=None` builds the array on the device (SuffixArray::new without downloading it)."""

    def __init__(self, s, sa: Optional[np.ndarray] = None):
        self._s = _as_u8(s)
        h = ctypes.c_void_p()
        a = None if sa is None else np.ascontiguousarray(sa, dtype=np.uint32)
        if a is not None:
            assert a.size == self._s.size + 1
        self._lib = lib()              # the library that made the handle destroys it, whichever one lib() answers by then
        _check(self._lib.sa_amd_index_create(self._s.ctypes.data, self._s.size, None if a is None else a.ctypes.data,
                                             ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sa_amd_index_destroy(self._h)
            self._h = None

    __del__ = close

    def suffix_array(self) -> np.ndarray:
        out = np.empty(self._s.size + 1, dtype=np.uint32)
        _check(lib().sa_amd_index_sa(self._h, out.ctypes.data))
        return out

    def buckets(self) -> np.ndarray:
        bkt = np.empty(BUCKET_TABLE_LEN, dtype=np.uint32)
        _check(lib().sa_amd_index_buckets(self._h, bkt.ctypes.data))
        return bkt

    def check_integrity(self) -> bool:
        rc = lib().sa_amd_index_check_integrity(self._h)
        if rc < 0 and rc != -6:
            _check(rc)
        return rc == 1

    def lcp(self) -> np.ndarray:
        """LCP array of the resident text and suffix array (see ``lcp``)"""
        out = np.empty(self._s.size + 1, dtype=np.uint32)
        _lcp_rc(lib().sa_amd_index_lcp(self._h, out.ctypes.data))
        return out

    def bwt(self):
        """-> (b, primary): the Burrows-Wheeler transform from the resident text and suffix array (see ``bwt``)"""
        out = np.empty(self._s.size, dtype=np.uint8)
        primary = ctypes.c_int32(0)
        _bwt_rc(lib().sa_amd_index_bwt(self._h, out.ctypes.data, ctypes.byref(primary)))
        return out, int(primary.value)

    def repeat_lengths(self) -> np.ndarray:
        """longest-repeat array from the resident text and suffix array (see ``repeat_lengths``)"""
        out = np.empty(self._s.size, dtype=np.uint32)
        _bwt_rc(lib().sa_amd_index_repeat_lengths(self._h, out.ctypes.data))
        return out

    def repeat_spans(self, min_len: int, keep_first: bool = False) -> np.ndarray:
        """duplicate spans from the resident text and suffix array (see ``repeat_spans``)"""
        k = _repeat_min_len(min_len)
        cap = (self._s.size + 1) // (k + 1)
        out = np.empty((cap, 2), dtype=np.uint32)
        count = ctypes.c_int64(0)
        _bwt_rc(lib().sa_amd_index_repeat_spans(self._h, k, REPEATS_KEEP_FIRST if keep_first else REPEATS_ALL, out.ctypes.data, cap,
                                                ctypes.byref(count)))
        return out[:min(int(count.value), cap)].copy()

    def lpf(self):
        """``(LPF, SRC)`` from the resident text and suffix array (see ``lpf``)"""
        out = np.empty((2, self._s.size), dtype=np.uint32)
        _bwt_rc(lib().sa_amd_index_lpf(self._h, out[0].ctypes.data, out[1].ctypes.data))
        return out[0], out[1]

    def lz77(self) -> np.ndarray:
        """the LZ77 parse from the resident text and suffix array (see ``lz77``)"""
        cap = min(self._s.size, max(1 << 16, self._s.size // 8))
        while True:
            out = np.empty((cap, 2), dtype=np.uint32)
            count = ctypes.c_int64(0)
            _bwt_rc(lib().sa_amd_index_lz77(self._h, out.ctypes.data, cap, ctypes.byref(count)))
            if count.value <= cap:
                return out[:int(count.value)].copy()
            cap = int(count.value)

    def repeated_substrings(self, min_len: int = 1, max_len: int = 0, min_count: int = 2, order: int = SUBSTR_ALL, k: int = 0,
                            positions: bool = False):
        """EXTENSION (the reference lacks it): the repeated substrings from the resident text and suffix array, all of them or
        the best ``k`` (see ``repeated_substrings``)"""
        q = SubstrQuery(int(min_len), int(max_len), int(min_count), int(order), int(k))
        return _substr_rows(self._s.size, q, positions, lambda qp, rp, pp, cap, tot: lib().sa_amd_index_substrings(self._h, qp, rp, pp, cap, tot))

    def doc_substrings(self, min_len: int = 1, max_len: int = 0, min_count: int = 2, min_docs: int = 1, order: int = SUBSTR_ALL, k: int = 0,
                       positions: bool = False):
        """EXTENSION: the repeated substrings with their document frequency -> ``(rows, df)`` or ``(rows, df, pos)``.  ``rows``
        and ``pos`` as ``repeated_substrings`` returns them; ``df[r]`` is the number of distinct documents of the collection
        (``set_documents``) that an occurrence of row ``r``'s substring starts in.  A node is selected when the filter of
        ``repeated_substrings`` holds and ``df >= min_docs``; ``SUBSTR_BY_DOCS`` ranks by ``df``, ties in suffix-array order.  A
        substring may cross a document boundary, as a pattern of ``doc_search`` may."""
        q = DocSubstrQuery(int(min_len), int(max_len), int(min_count), int(order), int(k), int(min_docs))
        n = self._s.size
        bound = max(n - 1, 0)
        cap = min(bound, int(q.k)) if q.order != SUBSTR_ALL and q.k >= 1 else min(bound, max(1 << 16, n // 8))
        while True:
            rows = np.empty((cap, 4), dtype=np.uint32)
            df = np.empty(cap, dtype=np.uint32)
            pos = np.empty(cap, dtype=np.uint32) if positions else None
            total = ctypes.c_int64(0)
            _bwt_rc(lib().sa_amd_index_doc_substrings(self._h, ctypes.byref(q), rows.ctypes.data if cap else None, df.ctypes.data if cap else None,
                                                      pos.ctypes.data if positions and cap else None, cap, ctypes.byref(total)))
            if total.value <= cap:
                m = int(total.value)
                return (rows[:m].copy(), df[:m].copy(), pos[:m].copy()) if positions else (rows[:m].copy(), df[:m].copy())
            cap = int(total.value)

    def match_stats(self, query, max_len: int):
        """-> ``(ml, pos)``, uint32 arrays over the positions of ``query``: ``ml[j]`` is the length, capped at ``max_len``, of the
        longest prefix of ``query[j:]`` that occurs in the indexed text, ``pos[j]`` a place where it occurs (``MATCH_NONE`` where
        ``ml[j] == 0``) -- the neighbour of the window's insertion point in the suffix array with the longer match, the right
        one on a tie.  The same answers with or without the bucket and LCP tables."""
        q = _as_u8(query)
        assert q.size <= MAX_LENGTH
        cap = min(_repeat_min_len(max_len), 2**31 - 1)
        out = np.empty((2, q.size), dtype=np.uint32)
        _check(lib().sa_amd_index_match_stats(self._h, q.ctypes.data, q.size, cap, out[0].ctypes.data, out[1].ctypes.data))
        return out[0], out[1]

    def match_spans(self, query, min_len: int) -> np.ndarray:
        """the byte ranges of ``query`` covered by substrings of at least ``min_len`` bytes that occur in the indexed text: a
        ``(count, 2)`` uint32 array of ``[start, end)`` rows, ascending, disjoint and not adjacent.  Only the spans come back
        from the device."""
        q = _as_u8(query)
        assert q.size <= MAX_LENGTH
        k = _repeat_min_len(min_len)
        cap = (q.size + 1) // (k + 1)
        out = np.empty((cap, 2), dtype=np.uint32)
        count = ctypes.c_int64(0)
        _check(lib().sa_amd_index_match_spans(self._h, q.ctypes.data, q.size, k, out.ctypes.data, cap, ctypes.byref(count)))
        return out[:min(int(count.value), cap)].copy()

    def set_documents(self, offsets) -> None:
        """EXTENSION: make the text a collection of documents.  ``offsets``: ``ndocs + 1`` non-decreasing values from 0 to
        ``len(text)``; document ``d`` is ``text[offsets[d]:offsets[d + 1]]`` (empty documents are legal).  Replaces an earlier
        collection; malformed offsets raise and leave it in place."""
        off = np.ascontiguousarray(offsets)
        if off.ndim != 1 or off.size < 2 or (off.size and (off.min() < 0 or off.max() > 0xFFFFFFFF)):
            raise SuffixArrayError(-1, "document offsets: ndocs + 1 values in 0 .. len(text)")
        off = off.astype(np.uint32)
        _check(lib().sa_amd_index_set_documents(self._h, off.ctypes.data, off.size - 1))
        self._ndocs = off.size - 1

    def doc_of(self, positions) -> np.ndarray:
        """the document each text position lies in (uint32; ``DOC_NONE`` for positions ``>= len(text)``, so the ``pos`` of
        ``match_stats`` can be passed as it is)"""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).ravel()
        out = np.empty(pos.size, dtype=np.uint32)
        _check(lib().sa_amd_index_doc_of(self._h, pos.ctypes.data, pos.size, out.ctypes.data))
        return out

    def doc_search(self, patterns):
        """-> ``(occ, df)``, uint32 arrays over the patterns: occurrences, and the number of distinct documents an occurrence
        starts in"""
        data, off, cnt = _pattern_batch(patterns)
        out = np.zeros((2, cnt), dtype=np.uint32)
        _check(lib().sa_amd_index_doc_search(self._h, data.ctypes.data, off.ctypes.data, cnt, out[0].ctypes.data, out[1].ctypes.data))
        return out[0], out[1]

    def doc_repeat_spans(self, min_len: int, mode: int = REPEATS_KEEP_FIRST, scope: int = DOCREP_OTHER, doc_bytes: bool = False):
        """EXTENSION: duplicate spans that respect the document boundaries, in the form ``repeat_spans`` returns them.  A window
        of ``min_len`` bytes counts only where it lies inside its document; it is flagged when the same window occurs at
        another such position (``DOCREP_ANY``) or in another document (``DOCREP_OTHER``) -- anywhere (``REPEATS_ALL``) or earlier
        (``REPEATS_KEEP_FIRST``: the first copy survives).  ``doc_bytes=True`` returns ``(spans, doc_bytes)`` with the covered
        bytes of every document (uint32, ``ndocs`` entries)."""
        k = _repeat_min_len(min_len)
        ndocs = getattr(self, "_ndocs", 0)
        if ndocs < 1:
            raise SuffixArrayError(-1, "doc_repeat_spans: set_documents first")
        cap = (self._s.size + 1) // (k + 1)
        out = np.empty((cap, 2), dtype=np.uint32)
        db = np.zeros(ndocs, dtype=np.uint32) if doc_bytes else None
        count = ctypes.c_int64(0)
        _bwt_rc(lib().sa_amd_index_doc_repeat_spans(self._h, k, int(mode), int(scope), out.ctypes.data, cap, ctypes.byref(count),
                                                    None if db is None else db.ctypes.data))
        spans = out[:min(int(count.value), cap)].copy()
        return (spans, db) if doc_bytes else spans

    def doc_list(self, patterns) -> list:
        """-> per pattern the uint32 array of the distinct documents it occurs in, ordered by the document's lexicographically
        smallest matching suffix"""
        data, off, cnt = _pattern_batch(patterns)
        loff = np.zeros(cnt + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        cap = 1 << 16
        while True:
            docs = np.empty(cap, dtype=np.uint32)
            _check(lib().sa_amd_index_doc_list(self._h, data.ctypes.data, off.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, cap,
                                               ctypes.byref(total)))
            if total.value <= cap:
                return [docs[loff[q]:loff[q + 1]].copy() for q in range(cnt)]
            cap = int(total.value)

    def doc_match(self, queries, clause_df: bool = False):
        """EXTENSION: Boolean document queries.  A query is a sequence of clauses that must all hold (AND); a clause is one
        pattern, a sequence of patterns of which any may occur (OR), or ``Not(...)`` of either.  -> ``df``, uint32 over the
        queries: the number of documents each query holds in; with ``clause_df=True`` -> ``(df, clause_df)``, the second over
        all clauses in the order given: the documents in each clause's own set.  A query without clauses holds in every
        document, empty ones included."""
        data, off, npat, coff, cfl, ncl, qoff, nq = _query_batch(queries)
        df = np.zeros(nq, dtype=np.uint32)
        cdf = np.zeros(ncl, dtype=np.uint32) if clause_df else None
        _check(lib().sa_amd_index_doc_match(self._h, data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl,
                                            qoff.ctypes.data, nq, df.ctypes.data if nq else None,
                                            cdf.ctypes.data if clause_df and ncl else None))
        return (df, cdf) if clause_df else df

    def doc_match_list(self, queries) -> list:
        """EXTENSION: per query of ``doc_match`` the uint32 array of the documents it holds in, in ascending document id"""
        data, off, npat, coff, cfl, ncl, qoff, nq = _query_batch(queries)
        loff = np.zeros(nq + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        cap = 1 << 16
        while True:
            docs = np.empty(cap, dtype=np.uint32)
            _check(lib().sa_amd_index_doc_match_list(self._h, data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl,
                                                     qoff.ctypes.data, nq, loff.ctypes.data, docs.ctypes.data, cap, ctypes.byref(total)))
            if total.value <= cap:
                return [docs[loff[q]:loff[q + 1]].copy() for q in range(nq)]
            cap = int(total.value)

    def enable_doc_freq(self) -> None:
        """EXTENSION: build and keep the slots ordered by document (4 bytes per byte of text) that ``doc_tf`` and ``doc_topk``
        need.  A no-op when the table exists; ``set_documents`` drops it, so enable it again after replacing the collection."""
        _check(lib().sa_amd_index_enable_doc_freq(self._h))

    def doc_tf(self, patterns) -> list:
        """-> per pattern ``(docs, tf)``: the listing of ``doc_list`` and, next to every document, the number of occurrences
        that start in it (uint32 arrays)"""
        data, off, cnt = _pattern_batch(patterns)
        loff = np.zeros(cnt + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        cap = 1 << 16
        while True:
            out = np.empty((2, cap), dtype=np.uint32)
            _check(lib().sa_amd_index_doc_tf(self._h, data.ctypes.data, off.ctypes.data, cnt, loff.ctypes.data, out[0].ctypes.data,
                                             out[1].ctypes.data, cap, ctypes.byref(total)))
            if total.value <= cap:
                return [(out[0, loff[q]:loff[q + 1]].copy(), out[1, loff[q]:loff[q + 1]].copy()) for q in range(cnt)]
            cap = int(total.value)

    def doc_topk(self, patterns, k: int) -> list:
        """-> per pattern ``(docs, tf)``: the ``min(k, df)`` documents with the most occurrences, by ``tf`` descending and then by
        document id ascending (uint32 arrays); ``1 <= k <= DOC_TOPK_MAX``"""
        data, off, cnt = _pattern_batch(patterns)
        k = int(k)
        if not 1 <= k <= DOC_TOPK_MAX:
            raise SuffixArrayError(-1, "doc_topk: k in 1 .. DOC_TOPK_MAX")
        toff = np.zeros(cnt + 1, dtype=np.int64)
        out = np.empty((2, max(cnt * k, 1)), dtype=np.uint32)
        _check(lib().sa_amd_index_doc_topk(self._h, data.ctypes.data, off.ctypes.data, cnt, k, toff.ctypes.data, out[0].ctypes.data,
                                           out[1].ctypes.data))
        return [(out[0, toff[q]:toff[q + 1]].copy(), out[1, toff[q]:toff[q + 1]].copy()) for q in range(cnt)]

    def _ngram(self, patterns, backoff: bool, min_count: int, max_len: int):
        batch = _pattern_batch(patterns)
        return _ngram_query(lib().sa_amd_index_next_bytes, lib().sa_amd_index_infgram, self._h, batch, np.uint8,
                            min(256 * batch[2], max(1 << 16, 8 * batch[2])), backoff, min_count, max_len)

    def next_bytes(self, patterns, dense: bool = False):
        """EXTENSION: what follows each context in the text, and how often -> ``(lo, hi, at_end, list_off, bytes, counts)``.
        ``[lo, hi)`` is the context's match range (``search``), ``at_end`` is 1 where the context is a suffix of the text, and the
        listing of context ``q`` is ``bytes[list_off[q]:list_off[q + 1]]`` (ascending) with ``counts`` next to it: the number of
        occurrences followed by that byte.  ``sum(counts) + at_end == hi - lo``, and the occurrences followed by ``b`` are the
        sub-range that starts at ``lo + at_end`` plus the counts of the smaller bytes.  ``dense=True`` -> ``(lo, hi, at_end, next)``
        with ``next`` a ``(count, 256)`` uint32 array, filled on the host from the sparse result."""
        _, lo, hi, ae, loff, b, c = self._ngram(patterns, False, 1, 0)
        if not dense:
            return lo, hi, ae, loff, b, c
        nxt = np.zeros((lo.size, 256), dtype=np.uint32)
        nxt[np.repeat(np.arange(lo.size), np.diff(loff)), b] = c
        return lo, hi, ae, nxt

    def infgram(self, prompts, min_count: int = 1, max_len: int = 0):
        """EXTENSION: the infinity-gram query -> ``(suffix_len, lo, hi, at_end, list_off, bytes, counts)``.  ``suffix_len[q]`` is the
        length ``s`` of the longest suffix of prompt ``q`` -- of at most ``max_len`` bytes where ``max_len > 0`` -- that occurs at
        least ``min_count`` times; ``s = 0`` (the unigram distribution) always qualifies.  The other outputs are those of
        ``next_bytes`` for that suffix."""
        if int(min_count) < 1:
            raise SuffixArrayError(-1, "infgram: min_count >= 1")
        return self._ngram(prompts, True, min(int(min_count), 2**31 - 1), max(0, min(int(max_len), 2**31 - 1)))

    def infgram_score(self, query, min_count: int = 1, max_len: int = SCORE_MAX_CONTEXT, doc_offsets=None) -> ScoreResult:
        """EXTENSION: score ``query`` under the infinity-gram model -> ``ScoreResult``.  For every position ``j`` the context is
        the longest ``query[j - s:j]`` -- of at most ``max_len`` bytes (1 .. ``SCORE_MAX_CONTEXT``), never reaching back over the
        start of ``j``'s document -- that occurs at least ``min_count`` times: exactly ``infgram`` of the prompt
        ``query[start:j]``.  ``s``, ``lo`` / ``hi`` / ``at_end`` describe it, ``[nlo, nhi)`` is the part of its range that
        ``query[j]`` follows (empty, at its insertion point, where it never does).  ``doc_offsets``: ``ndocs + 1`` non-decreasing
        values from 0 to ``len(query)``; ``None`` is one document.  The query is read once on the device."""
        q = _as_u8(query)
        if int(min_count) < 1:
            raise SuffixArrayError(-1, "infgram_score: min_count >= 1")
        off, ndocs = _score_offsets(doc_offsets)
        m = int(q.size)
        s, lo, hi, nlo, nhi = (np.zeros(m, dtype=np.uint32) for _ in range(5))
        ae = np.zeros(m, dtype=np.uint8)
        _check(lib().sa_amd_index_infgram_score(self._h, q.ctypes.data if m else None, m, off.ctypes.data if off is not None else None, ndocs,
                                                min(int(min_count), 2**31 - 1), max(-1, min(int(max_len), 2**31 - 1)), s.ctypes.data, lo.ctypes.data,
                                                hi.ctypes.data, ae.ctypes.data, nlo.ctypes.data, nhi.ctypes.data))
        return ScoreResult(s, lo, hi, ae, nlo, nhi)

    def enable_lcp(self) -> None:
        """EXTENSION (the reference's README TODO "speed up searching by LCP array"): build and keep the LCP table of the
        search tree (8 (n + 1) bytes); later searches take the LCP route with the same answers.  A no-op when it exists."""
        _lcp_rc(lib().sa_amd_index_enable_lcp(self._h))

    def search(self, patterns):
        """-> dict of arrays over the patterns: contains (bool), lo/hi (search_all == sa[lo:hi]),
        lcp_start/lcp_len (search_lcp == start..start+len)"""
        pats = [bytes(p) for p in patterns]
        cnt = len(pats)
        off = np.zeros(cnt + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in pats])
        data = np.frombuffer(b"".join(pats), dtype=np.uint8) if off[-1] else np.zeros(1, dtype=np.uint8)
        c = np.zeros(cnt, dtype=np.uint8)
        lo, hi, ls, ll = (np.zeros(cnt, dtype=np.uint32) for _ in range(4))
        _check(lib().sa_amd_index_search(self._h, data.ctypes.data, off.ctypes.data, cnt, c.ctypes.data, lo.ctypes.data,
                                         hi.ctypes.data, ls.ctypes.data, ll.ctypes.data))
        return {"contains": c.astype(bool), "lo": lo, "hi": hi, "lcp_start": ls, "lcp_len": ll}


def _as_tokens(tokens, what: str, dtype, limit: int, check_array: bool = False) -> np.ndarray:
    """an array of ``dtype`` as it is, or a sequence of ints in 0 .. limit - 1 -> contiguous 1-D ``dtype``; anything else raises
    before the library is called.  ``check_array``: the values of an array are checked against ``limit`` too"""
    kind = f"a 1-D {np.dtype(dtype).name} array or a sequence of ints in 0 .. {limit - 1}"
    if isinstance(tokens, np.ndarray):
        if tokens.dtype != dtype or tokens.ndim != 1:
            raise TypeError(f"{what}: {kind}")
        if check_array and tokens.size and int(tokens.max()) >= limit:
            raise ValueError(f"{what}: token {int(tokens.max())} is outside 0 .. {limit - 1}")
        return np.ascontiguousarray(tokens)
    if isinstance(tokens, (bytes, bytearray, str)):
        raise TypeError(f"{what}: {kind}, not {type(tokens).__name__}")
    vals = list(tokens)
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{what}: {v!r} is not an int")
        if not 0 <= int(v) < limit:
            raise ValueError(f"{what}: token {int(v)} is outside 0 .. {limit - 1}")
    return np.array(vals, dtype=dtype).reshape(-1)


def _as_u16(tokens, what: str = "tokens") -> np.ndarray:
    """a uint16 array as it is, or a sequence of ints in 0 .. 65 535 -> contiguous 1-D uint16; anything else raises before the
    library is called"""
    return _as_tokens(tokens, what, np.uint16, 1 << 16)


def _as_u32(tokens, what: str = "tokens", text: bool = False) -> np.ndarray:
    """a uint32 array as it is, or a sequence of ints in 0 .. 2^24 - 1 -> contiguous 1-D uint32; anything else raises before the
    library is called.  The ids of an array are checked here unless it is a ``text``, whose ids the device checks (an id of 2^24
    or more is the library's SA_AMD_ERANGE)"""
    return _as_tokens(tokens, what, np.uint32, TOKEN_LIMIT_U32, check_array=not text)


def _batch_of(pats, dtype):
    off = np.zeros(len(pats) + 1, dtype=np.int64)
    off[1:] = np.cumsum([p.size for p in pats])
    data = np.concatenate(pats) if off[-1] else np.zeros(1, dtype=dtype)
    return np.ascontiguousarray(data, dtype=dtype), off, len(pats)


def _is_token_pattern(x) -> bool:
    """one token pattern: a 1-D array, or a non-empty list or tuple of ints (an empty list is a clause without patterns, as for
    ``DeviceIndex``; the empty pattern is an empty array)"""
    if isinstance(x, np.ndarray):
        return x.ndim == 1
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in x)


def _token_batch(patterns):
    return _batch_of([_as_u16(p, "pattern") for p in patterns], np.uint16)


def _token_batch32(patterns):
    return _batch_of([_as_u32(p, "pattern") for p in patterns], np.uint32)


def saca_u16(tokens) -> np.ndarray:
    """EXTENSION: the suffix array of a text of 16-bit tokens (``sa_amd_saca_u16``) -> uint32 array of ``n + 1`` entries in
    token positions, entry 0 is ``n``.  Tokens compare as unsigned 16-bit values; a suffix that is a prefix of another sorts
    first.  Built on the GPU from the big-endian byte image of the tokens; only the final array comes down."""
    t = _as_u16(tokens)
    if t.size > MAX_TOKENS_U16:
        raise ValueError(f"saca_u16: at most {MAX_TOKENS_U16} tokens")
    out = np.empty(t.size + 1, dtype=np.uint32)
    _check(lib().sa_amd_saca_u16(t.ctypes.data if t.size else None, out.ctypes.data, t.size))
    return out


def saca_u32(tokens) -> np.ndarray:
    """EXTENSION: the suffix array of a text of token ids below 2^24 held in uint32 (``sa_amd_saca_u32``) -> uint32 array of
    ``n + 1`` entries in token positions, entry 0 is ``n``: ``saca_u16`` for the vocabularies that do not fit 16 bits.  Built on
    the GPU from the big-endian image at three bytes a token; an id of 2^24 or more in an array is found there
    (``SuffixArrayError``, SA_AMD_ERANGE), in a sequence of ints here (``ValueError``)."""
    t = _as_u32(tokens, text=True)
    if t.size > MAX_TOKENS_U32:
        raise ValueError(f"saca_u32: at most {MAX_TOKENS_U32} tokens")
    out = np.empty(t.size + 1, dtype=np.uint32)
    _check(lib().sa_amd_saca_u32(t.ctypes.data if t.size else None, out.ctypes.data, t.size))
    return out


def last_tok_stats() -> dict:
    """the query counters of this thread's most recent ``TokenIndex.next_tokens`` / ``.infgram`` call (the fields of
    ``last_ngram_stats``, ``compared_tokens`` in place of ``compared_bytes``) and image_ms / build_ms / compact_ms of its most
    recent token build"""
    st = TokStats()
    lib().sa_amd_last_tok_stats(ctypes.byref(st))
    return st.as_dict()


def last_tok_score_stats() -> dict:
    """the counters of this thread's most recent ``TokenIndex.infgram_score`` call: the keys of ``last_score_stats`` with
    ``compared_tokens`` in place of ``compared_bytes``; no other call writes them"""
    st = TokScoreStats()
    lib().sa_amd_last_tok_score_stats(ctypes.byref(st))
    return st.as_dict()


class TokenIndex:
    """EXTENSION: a text of 16-bit tokens and its suffix array resident in HBM (sa_amd_tok_index of
    include/suffix_array_amd.h): batched range search, next-token counts and the infinity-gram back-off.  ``sa=None`` builds the
    array on the device without downloading it; a supplied array is range-checked.  Patterns are sequences of uint16 arrays
    or of sequences of ints in 0 .. 65 535; every length and offset is in tokens."""

    # what TokenIndex32 replaces: the prefix of the ABI's names, the token type, the longest text, the coercions
    _abi = "sa_amd_tok_index_"
    _dtype = np.uint16
    _max_tokens = MAX_TOKENS_U16
    _as_text = staticmethod(lambda tokens: _as_u16(tokens))
    _as_query = staticmethod(lambda tokens: _as_u16(tokens, "query"))
    _batch = staticmethod(lambda patterns: _token_batch(patterns))

    def _fn(self, op: str, library=None):
        return getattr(library or lib(), self._abi + op)

    def __init__(self, tokens, sa: Optional[np.ndarray] = None):
        name = type(self).__name__
        self._t = self._as_text(tokens)
        if self._t.size > self._max_tokens:
            raise ValueError(f"{name}: at most {self._max_tokens} tokens")
        a = None if sa is None else np.ascontiguousarray(sa, dtype=np.uint32)
        if a is not None and a.size != self._t.size + 1:
            raise ValueError(f"{name}: sa has len(tokens) + 1 entries")
        h = ctypes.c_void_p()
        self._lib = lib()              # (as DeviceIndex: destroyed through the library that made it)
        _check(self._fn("create", self._lib)(self._t.ctypes.data if self._t.size else None, self._t.size,
                                             None if a is None else a.ctypes.data, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy", self._lib)(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return int(self._t.size)

    def sa(self) -> np.ndarray:
        out = np.empty(self._t.size + 1, dtype=np.uint32)
        _check(self._fn("sa")(self._h, out.ctypes.data))
        return out

    def _search(self, patterns, contains: bool):
        data, off, cnt = self._batch(patterns)
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32)
        has = np.zeros(cnt, dtype=np.uint8)
        _check(self._fn("search")(self._h, data.ctypes.data, off.ctypes.data, cnt, has.ctypes.data if contains else None,
                                  lo.ctypes.data, hi.ctypes.data))
        return has, lo, hi

    def search(self, patterns):
        """-> ``(lo, hi)``: the match range of every pattern in the token suffix array; ``lo == hi`` where it does not occur"""
        _, lo, hi = self._search(patterns, False)
        return lo, hi

    def count(self, patterns) -> np.ndarray:
        """occurrences of every pattern (``hi - lo``; the empty pattern has ``n + 1``)"""
        lo, hi = self.search(patterns)
        return hi.astype(np.int64) - lo.astype(np.int64)

    def contains(self, patterns) -> np.ndarray:
        return self._search(patterns, True)[0].astype(bool)

    def _ngram(self, patterns, backoff: bool, min_count: int, max_len: int):
        batch = self._batch(patterns)
        return _ngram_query(self._fn("next_tokens"), self._fn("infgram"), self._h, batch, self._dtype,
                            max(1 << 16, 8 * batch[2]), backoff, min_count, max_len)

    def next_tokens(self, patterns):
        """what follows each context in the text, and how often -> ``(lo, hi, at_end, list_off, tokens, counts)``, the result
        shape of ``DeviceIndex.next_bytes`` with tokens in place of bytes: the listing of context ``q`` is
        ``tokens[list_off[q]:list_off[q + 1]]`` (ascending) with ``counts`` next to it, ``sum(counts) + at_end == hi - lo``, and the
        occurrences followed by ``t`` are the sub-range that starts at ``lo + at_end`` plus the counts of the smaller tokens."""
        return self._ngram(patterns, False, 1, 0)[1:]

    def infgram(self, prompts, min_count: int = 1, max_len: int = 0):
        """the infinity-gram query -> ``(suffix_len, lo, hi, at_end, list_off, tokens, counts)``: ``suffix_len[q]`` is the length in
        tokens of the longest suffix of prompt ``q`` -- of at most ``max_len`` tokens where ``max_len > 0`` -- that occurs at least
        ``min_count`` times; the other outputs are those of ``next_tokens`` for that suffix."""
        if int(min_count) < 1:
            raise SuffixArrayError(-1, "infgram: min_count >= 1")
        return self._ngram(prompts, True, min(int(min_count), 2**31 - 1), max(0, min(int(max_len), 2**31 - 1)))

    def infgram_score(self, query, min_count: int = 1, max_len: int = SCORE_MAX_CONTEXT, doc_offsets=None) -> ScoreResult:
        """score a token ``query`` under the infinity-gram model -> ``ScoreResult`` (``DeviceIndex.infgram_score`` with tokens in
        place of bytes).  For every position ``j`` the context is the longest ``query[j - s:j]`` -- of at most ``max_len`` tokens
        (1 .. ``SCORE_MAX_CONTEXT``), never reaching back over the start of ``j``'s document -- that occurs at least
        ``min_count`` times: exactly ``infgram`` of the prompt ``query[start:j]``.  ``s``, ``lo`` / ``hi`` / ``at_end`` describe
        it, ``[nlo, nhi)`` is the part of its range that ``query[j]`` follows (empty, at its insertion point, where it never
        does).  ``doc_offsets``: ``ndocs + 1`` non-decreasing values from 0 to ``len(query)``, in tokens; ``None`` is one
        document.  The query (2 bytes a token) is read once on the device; ``score_set_group_cap`` applies, counted in tokens."""
        q = self._as_query(query)
        if int(min_count) < 1:
            raise SuffixArrayError(-1, "infgram_score: min_count >= 1")
        off, ndocs = _score_offsets(doc_offsets)
        m = int(q.size)
        s, lo, hi, nlo, nhi = (np.zeros(m, dtype=np.uint32) for _ in range(5))
        ae = np.zeros(m, dtype=np.uint8)
        _check(self._fn("infgram_score")(self._h, q.ctypes.data if m else None, m, off.ctypes.data if off is not None else None, ndocs,
                                         min(int(min_count), 2**31 - 1), max(-1, min(int(max_len), 2**31 - 1)), s.ctypes.data,
                                         lo.ctypes.data, hi.ctypes.data, ae.ctypes.data, nlo.ctypes.data, nhi.ctypes.data))
        return ScoreResult(s, lo, hi, ae, nlo, nhi)

    # ---- document collections (include/sa_amd_tokdocs.h): the methods of ``DeviceIndex`` with tokens for bytes ----

    def set_documents(self, offsets=None, *, separator=None) -> int:
        """EXTENSION: make the text a collection of documents -> ``ndocs``.  Exactly one of the two: ``offsets``, ``ndocs + 1``
        non-decreasing values from 0 to ``len(self)`` in tokens (document ``d`` is ``tokens[offsets[d]:offsets[d + 1]]``, empty
        documents are legal), or ``separator``, a token id: every occurrence ends a document and belongs to it, found on the
        device in the resident text; what follows the last one is a last document.  Replaces an earlier collection; a call that
        fails leaves it in place."""
        if (offsets is None) == (separator is None):
            raise TypeError("set_documents: exactly one of offsets and separator")
        if separator is not None:
            if isinstance(separator, bool) or not isinstance(separator, (int, np.integer)) or not 0 <= int(separator) <= 0xFFFFFFFF:
                raise TypeError("set_documents: separator is a token id")
            nd = ctypes.c_int64(0)
            _check(self._fn("set_documents_by_separator")(self._h, int(separator), ctypes.byref(nd)))
            return int(nd.value)
        off = np.ascontiguousarray(offsets)
        if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu" or off.min() < 0 or off.max() > 0xFFFFFFFF:
            raise SuffixArrayError(-1, "document offsets: ndocs + 1 integers in 0 .. len(tokens)")
        off = off.astype(np.uint32)
        _check(self._fn("set_documents")(self._h, off.ctypes.data, off.size - 1))
        return off.size - 1

    @property
    def ndocs(self) -> int:
        """documents of the collection in effect, as the library holds it (no copy is kept here); 0 before ``set_documents``"""
        nd = ctypes.c_int64(0)
        rc = self._fn("doc_offsets")(self._h, None, 0, ctypes.byref(nd))
        if rc == -1:                                                  # SA_AMD_EINVAL: no collection yet
            return 0
        _check(rc)
        return int(nd.value)

    def doc_offsets(self) -> np.ndarray:
        """the collection in effect as ``set_documents`` takes it: ``ndocs + 1`` offsets in tokens (uint32), from the device"""
        nd = ctypes.c_int64(0)
        _check(self._fn("doc_offsets")(self._h, None, 0, ctypes.byref(nd)))
        out = np.empty(int(nd.value) + 1, dtype=np.uint32)
        _check(self._fn("doc_offsets")(self._h, out.ctypes.data, out.size, ctypes.byref(nd)))
        return out[:int(nd.value) + 1] if int(nd.value) + 1 <= out.size else self.doc_offsets()      # (replaced in between: again)

    def doc_of(self, positions) -> np.ndarray:
        """the document each token position lies in (uint32; ``DOC_NONE`` for positions ``>= len(self)``)"""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).ravel()
        out = np.empty(pos.size, dtype=np.uint32)
        _check(self._fn("doc_of")(self._h, pos.ctypes.data, pos.size, out.ctypes.data))
        return out

    def doc_search(self, patterns):
        """-> ``(occ, df)``, uint32 arrays over the patterns: occurrences (``hi - lo`` of ``search``), and the number of distinct
        documents an occurrence starts in"""
        data, off, cnt = self._batch(patterns)
        out = np.zeros((2, cnt), dtype=np.uint32)
        _check(self._fn("doc_search")(self._h, data.ctypes.data, off.ctypes.data, cnt, out[0].ctypes.data, out[1].ctypes.data))
        return out[0], out[1]

    def _doc_listing(self, fn, args, rows: int) -> list:
        loff = np.zeros(rows + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        cap = 1 << 16
        while True:
            docs = np.empty(cap, dtype=np.uint32)
            _check(fn(self._h, *args, loff.ctypes.data, docs.ctypes.data, cap, ctypes.byref(total)))
            if total.value <= cap:
                return [docs[loff[q]:loff[q + 1]].copy() for q in range(rows)]
            cap = int(total.value)

    def doc_list(self, patterns) -> list:
        """-> per pattern the uint32 array of the distinct documents it occurs in, ordered by the document's smallest matching
        suffix (slot order)"""
        data, off, cnt = self._batch(patterns)
        return self._doc_listing(self._fn("doc_list"), (data.ctypes.data, off.ctypes.data, cnt), cnt)

    def _queries(self, queries):
        return _query_batch(queries, _is_token_pattern, lambda p: p, self._batch)

    def doc_match(self, queries, clause_df: bool = False):
        """EXTENSION: Boolean document queries, the forms and results of ``DeviceIndex.doc_match``: a query is a sequence of
        clauses that must all hold; a clause is one token pattern (an array, or a non-empty list of ints), a sequence of
        patterns of which any may occur, or ``Not(...)`` of either.  -> ``df`` over the queries, with ``clause_df=True``
        ``(df, clause_df)``."""
        data, off, npat, coff, cfl, ncl, qoff, nq = self._queries(queries)
        df = np.zeros(nq, dtype=np.uint32)
        cdf = np.zeros(ncl, dtype=np.uint32) if clause_df else None
        _check(self._fn("doc_match")(self._h, data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl,
                                     qoff.ctypes.data, nq, df.ctypes.data if nq else None, cdf.ctypes.data if clause_df and ncl else None))
        return (df, cdf) if clause_df else df

    def doc_match_list(self, queries) -> list:
        """EXTENSION: per query of ``doc_match`` the uint32 array of the documents it holds in, in ascending document id"""
        data, off, npat, coff, cfl, ncl, qoff, nq = self._queries(queries)
        return self._doc_listing(self._fn("doc_match_list"),
                                 (data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl, qoff.ctypes.data, nq), nq)


class TokenIndex32(TokenIndex):
    """EXTENSION: ``TokenIndex`` for token ids below 2^24 held in uint32 (sa_amd_tok32_index of include/suffix_array_amd_tok32.h): the
    same methods with the same results, the listings' tokens as uint32, a query at 4 bytes a token.  ``tokens`` is a 1-D uint32
    array (an id of 2^24 or more is found on the device: ``SuffixArrayError``, SA_AMD_ERANGE) or a sequence of ints in
    0 .. 2^24 - 1; patterns, prompts and queries likewise, and an id of 2^24 or more in one of them is a ``ValueError`` before
    the library is called."""

    _abi = "sa_amd_tok32_index_"
    _dtype = np.uint32
    _max_tokens = MAX_TOKENS_U32
    _as_text = staticmethod(lambda tokens: _as_u32(tokens, text=True))
    _as_query = staticmethod(lambda tokens: _as_u32(tokens, "query"))
    _batch = staticmethod(lambda patterns: _token_batch32(patterns))


def workspace_bytes(n: int) -> int:
    return int(lib().sa_amd_workspace_bytes(n))


def saca_device_ptr(text_ptr: int, sa_ptr: int, n: int, work_ptr: int, work_bytes: int, stream: int = 0,
                    stats: Optional[Stats] = None) -> None:
    """Device-resident build (raw device pointers, e.g. torch ``tensor.data_ptr()``)."""
    _check(lib().sa_amd_saca_device(text_ptr, sa_ptr, n, work_ptr, work_bytes, stream,
                                    ctypes.byref(stats) if stats is not None else None))


def _check_integrity(s: np.ndarray, sa: np.ndarray) -> bool:
    """reference src/sa.rs:72-84, in its linear-time equivalent form:
    a length check, then every adjacent pair must be strictly increasing as byte slices.
    IndexError for an entry > n, also for the empty text (as the GPU check: see sa_amd_check_integrity)."""
    n = s.size
    if n + 1 != sa.size:                              # src/sa.rs:73-75
        return False
    if sa.max() > n:
        raise IndexError("suffix offset out of range (the reference panics here, src/sa.rs:77-78)")
    if n <= 64:                                       # literal form for tiny inputs
        return _check_integrity_literal(s, sa)
    return _check_integrity_linear(s, sa)


def _check_integrity_literal(s: np.ndarray, sa: np.ndarray) -> bool:
    """the pairwise slice comparison of src/sa.rs:76-82 (entries already known to be <= n)"""
    b = s.tobytes()
    return all(b[int(sa[i - 1]):] < b[int(sa[i]):] for i in range(1, s.size + 1))


def _check_integrity_linear(s: np.ndarray, sa: np.ndarray) -> bool:
    """the same answer in linear time: sa[0] = n, a permutation, first bytes then ranks of the next suffixes increasing
    (entries already known to be <= n)"""
    n = s.size
    if int(sa[0]) != n:
        return False
    rank = np.full(n + 1, -1, dtype=np.int64)
    rank[sa] = np.arange(n + 1)
    if (rank < 0).any():
        return False
    a, b = sa[1:-1].astype(np.int64), sa[2:].astype(np.int64)
    ca, cb = s[a], s[b]
    ok = (ca < cb) | ((ca == cb) & (rank[a + 1] < rank[b + 1]))
    return bool(ok.all())


class SuffixArray:
    """Mirror of ``SuffixArray<'a>`` for the construction path (reference src/sa.rs:13-70)."""

    def __init__(self, s):
        """``SuffixArray::new`` -- reference src/sa.rs:23-27."""
        self._s = _as_u8(s)
        self._sa = np.zeros(self._s.size + 1, dtype=np.uint32)     # vec![0; s.len() + 1]
        saca(self._s, self._sa)
        self._bkt = None
        self._esa = False
        self._ix = None

    @classmethod
    def new(cls, s) -> "SuffixArray":
        return cls(s)

    def set(self, s) -> None:
        """``SuffixArray::set`` -- reference src/sa.rs:30-33 (like the reference it re-runs
        construction into the resized buffer and leaves the stored text and buckets alone)."""
        t = _as_u8(s)
        self._sa = np.resize(self._sa, t.size + 1)
        saca(t, self._sa)
        self._ix = None                                # the device-resident index (a cache of this object) held the old array

    def fit(self) -> None:                             # src/sa.rs:36-38 (shrink_to_fit: numpy arrays carry no slack)
        self._sa = np.ascontiguousarray(self._sa)

    def as_ref(self) -> np.ndarray:                    # AsRef<[u8]>, src/sa.rs:370-374
        return self._s

    def len(self) -> int:                              # src/sa.rs:41-43
        return int(self._s.size)

    def is_empty(self) -> bool:                        # src/sa.rs:46-48
        return self.len() == 0

    def into_parts(self):                              # src/sa.rs:51-53
        return self._s, self._sa

    @classmethod
    def from_parts(cls, s, sa) -> Optional["SuffixArray"]:
        """reference src/sa.rs:57-64: compose and check integrity; None when the check fails."""
        obj = cls.unchecked_from_parts(s, sa)
        if lib().sa_amd_device_count() > 0:
            ok = check_integrity(obj._s, obj._sa)             # HIP kernels k_ci_scatter / k_ci_check
        else:
            ok = _check_integrity(obj._s, obj._sa)            # host glue when no device is visible
        return obj if ok else None

    @classmethod
    def unchecked_from_parts(cls, s, sa) -> "SuffixArray":   # src/sa.rs:68-70
        obj = cls.__new__(cls)
        obj._s = _as_u8(s)
        obj._sa = np.ascontiguousarray(sa, dtype=np.uint32)
        obj._bkt = None
        obj._esa = False
        obj._ix = None
        return obj

    # feature `pack`: reference src/sa.rs:255-361
    def dump_bytes(self) -> bytes:
        return pack(self._sa)

    def dump(self, file) -> None:
        file.write(self.dump_bytes())

    @classmethod
    def load_bytes(cls, s, blob: bytes) -> "SuffixArray":
        """reference src/sa.rs:349-361: unpack, then check the integrity; ValueError = the reference's InvalidData"""
        obj = cls.from_parts(s, unpack(blob))
        if obj is None:
            raise ValueError("inconsistent suffix array")
        return obj

    @classmethod
    def load(cls, s, file) -> "SuffixArray":
        return cls.load_bytes(s, file.read())

    def enable_buckets(self) -> None:
        """reference src/sa.rs:89-119; a no-op when the table exists (src/sa.rs:90-92)"""
        if self._bkt is None:
            self._bkt = bucket_table(self._s, self._sa)
            if getattr(self, "_ix", None) is not None:
                self._ix.buckets()                     # the resident index now narrows its searches (get_bucket, src/sa.rs:123-144)

    def buckets(self) -> Optional[np.ndarray]:
        return self._bkt

    # search: reference src/sa.rs:164-253, one pattern per call as in the reference (a batch of one on
    # the device-resident index; use DeviceIndex.search for many patterns)
    def _index(self) -> "DeviceIndex":
        if getattr(self, "_ix", None) is None:
            self._ix = DeviceIndex(self._s, self._sa)
            if self._bkt is not None:
                self._ix.buckets()
            if getattr(self, "_esa", False):
                self._ix.enable_lcp()
        return self._ix

    def contains(self, pat) -> bool:
        return bool(self._index().search([pat])["contains"][0])

    def search_all(self, pat) -> np.ndarray:
        r = self._index().search([pat])
        return self._sa[int(r["lo"][0]):int(r["hi"][0])]

    def search_lcp(self, pat) -> range:
        r = self._index().search([pat])
        return range(int(r["lcp_start"][0]), int(r["lcp_start"][0]) + int(r["lcp_len"][0]))

    def lcp_array(self) -> np.ndarray:
        """EXTENSION (the reference lacks it: its README's TODO "construct enhanced suffix array"): the LCP array aligned
        with the suffix array, ``lcp[0] == 0``, ``lcp[i]`` = longest common prefix of the suffixes at ``sa[i-1]`` and
        ``sa[i]``; computed on the GPU from the text and the array"""
        return lcp(self._s, self._sa)

    def bwt(self):
        """EXTENSION (the reference lacks it; ``divbwt`` of the C engine it binds): -> (b, primary), the Burrows-Wheeler
        transform from the text and the array, computed on the GPU (see ``bwt``)"""
        return bwt(self._s, self._sa)

    def repeat_lengths(self) -> np.ndarray:
        """EXTENSION (the reference lacks it): the longest-repeat array of the text, on the GPU (see ``repeat_lengths``)"""
        return repeat_lengths(self._s, self._sa)

    def repeat_spans(self, min_len: int, keep_first: bool = False) -> np.ndarray:
        """EXTENSION (the reference lacks it): the byte ranges that are copies, on the GPU (see ``repeat_spans``)"""
        return repeat_spans(self._s, min_len, keep_first, self._sa)

    def lpf(self):
        """EXTENSION (the reference lacks it): the longest-previous-factor array and its sources, on the GPU (see ``lpf``)"""
        return lpf(self._s, self._sa)

    def lz77(self) -> np.ndarray:
        """EXTENSION (the reference lacks it): the greedy LZ77 parse of the text, on the GPU (see ``lz77``)"""
        return lz77(self._s, self._sa)

    def repeated_substrings(self, min_len: int = 1, max_len: int = 0, min_count: int = 2, order: int = SUBSTR_ALL, k: int = 0,
                            positions: bool = False):
        """EXTENSION (the reference lacks it): the substrings that occur at least twice, all of them or the best ``k``, on the GPU
        (see ``repeated_substrings``)"""
        return repeated_substrings(self._s, min_len, max_len, min_count, order, k, self._sa, positions)

    def doc_substrings(self, min_len: int = 1, max_len: int = 0, min_count: int = 2, min_docs: int = 1, order: int = SUBSTR_ALL, k: int = 0,
                       positions: bool = False):
        """EXTENSION (the reference lacks it): the repeated substrings with their document frequency (see
        ``DeviceIndex.doc_substrings``)"""
        return self._index().doc_substrings(min_len, max_len, min_count, min_docs, order, k, positions)

    def match_stats(self, query, max_len: int):
        """EXTENSION (the reference lacks it): matching statistics of ``query`` against the text (see ``DeviceIndex.match_stats``)"""
        return self._index().match_stats(query, max_len)

    def match_spans(self, query, min_len: int) -> np.ndarray:
        """EXTENSION (the reference lacks it): the parts of ``query`` that occur in the text (see ``DeviceIndex.match_spans``)"""
        return self._index().match_spans(query, min_len)

    def set_documents(self, offsets) -> None:
        """EXTENSION (the reference lacks it): make the text a collection of documents (see ``DeviceIndex.set_documents``)"""
        self._index().set_documents(offsets)

    def doc_of(self, positions) -> np.ndarray:
        """EXTENSION (the reference lacks it): the document of each position (see ``DeviceIndex.doc_of``)"""
        return self._index().doc_of(positions)

    def doc_repeat_spans(self, min_len: int, mode: int = REPEATS_KEEP_FIRST, scope: int = DOCREP_OTHER, doc_bytes: bool = False):
        """EXTENSION (the reference lacks it): duplicate spans that respect the document boundaries (see
        ``DeviceIndex.doc_repeat_spans``)"""
        return self._index().doc_repeat_spans(min_len, mode, scope, doc_bytes)

    def doc_search(self, patterns):
        """EXTENSION (the reference lacks it): ``(occ, df)`` per pattern (see ``DeviceIndex.doc_search``)"""
        return self._index().doc_search(patterns)

    def doc_list(self, patterns) -> list:
        """EXTENSION (the reference lacks it): the documents each pattern occurs in (see ``DeviceIndex.doc_list``)"""
        return self._index().doc_list(patterns)

    def doc_match(self, queries, clause_df: bool = False):
        """EXTENSION (the reference lacks it): documents per Boolean query (see ``DeviceIndex.doc_match``)"""
        return self._index().doc_match(queries, clause_df)

    def doc_match_list(self, queries) -> list:
        """EXTENSION (the reference lacks it): the documents each Boolean query holds in (see ``DeviceIndex.doc_match_list``)"""
        return self._index().doc_match_list(queries)

    def enable_doc_freq(self) -> None:
        """EXTENSION (the reference lacks it): keep the table ``doc_tf`` / ``doc_topk`` need (see ``DeviceIndex.enable_doc_freq``)"""
        self._index().enable_doc_freq()

    def doc_tf(self, patterns) -> list:
        """EXTENSION (the reference lacks it): ``(docs, tf)`` per pattern (see ``DeviceIndex.doc_tf``)"""
        return self._index().doc_tf(patterns)

    def doc_topk(self, patterns, k: int) -> list:
        """EXTENSION (the reference lacks it): the ``k`` documents with the most occurrences per pattern (see
        ``DeviceIndex.doc_topk``)"""
        return self._index().doc_topk(patterns, k)

    def next_bytes(self, patterns, dense: bool = False):
        """EXTENSION (the reference lacks it): the bytes that follow each context and their counts (see
        ``DeviceIndex.next_bytes``)"""
        return self._index().next_bytes(patterns, dense)

    def infgram(self, prompts, min_count: int = 1, max_len: int = 0):
        """EXTENSION (the reference lacks it): the longest suffix of each prompt that occurs ``min_count`` times, and what
        follows it (see ``DeviceIndex.infgram``)"""
        return self._index().infgram(prompts, min_count, max_len)

    def infgram_score(self, query, min_count: int = 1, max_len: int = SCORE_MAX_CONTEXT, doc_offsets=None) -> ScoreResult:
        """EXTENSION (the reference lacks it): per-position back-off and next-byte counts of ``query`` under the infinity-gram
        model of the text (see ``DeviceIndex.infgram_score``)"""
        return self._index().infgram_score(query, min_count, max_len, doc_offsets)

    def enable_lcp(self) -> None:
        """EXTENSION (the reference's README TODO "speed up searching by LCP array"): contains / search_all / search_lcp
        from now on search over the LCP table of the device-resident index (DeviceIndex.enable_lcp), with the same answers;
        remembered like the bucket table, so the index that set() drops is rebuilt with it"""
        self._esa = True
        self._index().enable_lcp()

    def __array__(self, dtype=None):                   # From<SuffixArray> for Vec<u32>, src/sa.rs:364-368
        return self._sa if dtype is None else self._sa.astype(dtype)
