"""Every entry point that takes memory itself, with each of its memory requests refused in turn (the diagnostic library's switch).

All memory the library takes goes through three seams: a pooled device block (ResourcePool::acquire), a pinned host block
(ResourcePool::pinned) and a table of an index or a buffer of a host form (DevBuf::alloc).  sa_amd_debug_refuse_alloc
(csrc/sa_diag.h) makes the nth request of the calling thread ask the runtime for more bytes than any device has, so the runtime
itself says no and the thread is left as a real refusal leaves it.  CALLS has one entry per ABI call; the driver runs it on a
thread of its own (the switch, the pinned read-back block and its `failed` flag, the knobs and the runtime's last error are
thread_local):

  count-only pass (test_requests_of_a_call)   the requests of one successful call are the kinds the table states, 1 .. 64 of
      them; the answers are exact.  A call whose table entry states no request asserts that and stops.
  one case per request k (test_refused_request), ids call-k-kind:
   1  the refusal fired exactly once; the code is SA_AMD_OK or SA_AMD_ENOMEM, never anything else, and nothing is raised
   2  SA_AMD_ENOMEM: every output is byte for byte its canary (PARTIAL lists the exceptions, each with the header's sentence);
      an index under change passes its probe: it answers as before and the un-armed call then succeeds
   3  SA_AMD_OK: the answers are exact and (call, kind, k) is listed in FALLBACKS with its reason; an unlisted success fails,
      and so does a listed fallback that answers SA_AMD_ENOMEM
   4  hipPeekAtLastError() of the thread is hipSuccess after the call, whatever it returned
   5  the un-armed call that follows on the same thread is SA_AMD_OK with exact answers, and every work field of its
      statistics equals the count-only pass's (NOT_WORK and work_fields of tests/test_dirty_blocks.py)
   6  the thread gone, the case's indexes closed and the pool emptied, the ledger (sa_amd_debug_live_allocations) is what it
      was before the case

The answers come from the definitions of the features' own test files (imported, never a clean run of the library).  Sizes are
the smallest at which the routes still take their several blocks: test_streams.N = 70 001 bytes with the knobs of
tests/test_dirty_blocks.py, 4 097 bytes for the one-launch build, the token texts of tests/test_tokens.py, the 300 documents of
test_streams.DOC_OFF, and for the builds the general path, the staged download (SA_AMD_STAGED_MIN_BYTES=0) and the early download
of tests/test_dirty_blocks.py's BUILDS (3 MB, the only case above a few hundred kilobytes).

Out of reach of a per-thread switch, and said so in NO_CASE: what helper and worker threads request (the early pullers, the
workers of sa_amd_saca_batch); stream and event creation, which are no memory requests.

The CPU tests at the end keep CALLS complete against the headers and its parameters those of the declarations."""
import ctypes
import functools
import os

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
import dirty_blocks
import refused_allocs as ra
import test_dirty_blocks as tdb
import test_streams as ts
from conftest import ROOT
from refused_allocs import ENOMEM, OK, out
from test_bwt_abi import bwt_definition
from test_doc_match_abi import BUDGET_MIN
from test_doc_match_abi import match_definition as doc_match_definition
from test_doc_repeats_abi import doc_repeats_definition
from test_doc_substrings import model as doc_substrings_model
from test_doc_tf_abi import topk_definition
from test_docs import check_queries
from test_docs_abi import answers_definition as docs_answers_definition
from test_docs_abi import doc_of_definition
from test_gpu_parity import _hip
from test_lz77_abi import parse_definition
from test_ngram import check_outputs as check_ngram_outputs
from test_ngram_abi import infgram_definition
from test_substrings import model as substrings_model
from test_substrings_abi import ALL
from test_tok_score import composite_query
from test_tok_score import definition as tok_score_definition
from test_tok_score import text as token_text
from test_tok_score_abi import score_definition as tok_score_definition_lists
from test_tokens_abi import infgram_definition as tok_infgram_definition
from test_tokens_abi import next_tokens_definition
from test_tokens_abi import range_definition as tok_range_definition
import test_tokens as tk
import test_tokens32 as tk32
from test_tokens32_abi import reference_suffix_array32

N, MIN_LEN = ts.N, ts.MIN_LEN
READBACK = "read-back by copy: read_words remembers the refused pinned block for the thread and copies instead (host/readback.hpp)"
SMALLER = "the smaller integrity block: the streaming form's work block refused, the check runs in 4 (n + 1) + 256 bytes"
REDUCED = "the reduced-memory route: the full block refused, the build takes what the device has (host/host_path.hpp)"

# outputs a failing call may have written: call (a case's name, or the function without its prefix: all of its cases) ->
# (output, the header's sentence that allows it)
NULL_HANDLE = ("out", "a failing create sets *out to NULL, so that no caller is left with a dangling handle")
PARTIAL = {
    "index_create": NULL_HANDLE, "tok_index_create": NULL_HANDLE, "tok32_index_create": NULL_HANDLE,
    "index_doc_tf": ("tf", "a failing call can leave tf (partly) written and everything else untouched"),
    "index_doc_topk": ("tf", "a failing call can leave tf (partly) written and everything else untouched"),
    "saca_u8-early": ("SA", "a failing call can leave SA (partly) written once the early download has begun"),
    "unpack": ("length", "*length receives the stored length as soon as the header has been read, also where the call then fails"),
}


def T():
    return ts.text("real")[0]


def ARR():
    return ts.text("real")[1]


def TB():
    return T().tobytes()


def word(dtype=np.int64):
    return out(1, dtype)


def eq(got, exp):
    return tdb.eq(np.asarray(got), np.asarray(exp))


def rows_ok(a, want, count):
    """the first rows are `want`, the rest keeps the canary, the host word holds the number of all"""
    want = ts._u32(want)
    return prefix_ok(a, want) and int(count[0]) == want.shape[0]


def prefix_ok(a, want):
    """the flat output starts with `want` and keeps the canary behind it"""
    w = np.ascontiguousarray(want).reshape(-1)
    return a.dtype == w.dtype and eq(a[:w.size], w) and ra.untouched(a[w.size:])


class Ctx:
    """what a case works on: the indexes of the wrapper it made (closed with the case) and the handles its calls made"""

    def __init__(self, d):
        self.d, self.ix, self.tix, self.handles, self.extra = d, None, None, [], {}

    def index(self, tables=(), docs=False, freq=False, built=False):
        ix = self.d.index(T(), None if built else ARR())
        if "bkt" in tables:
            ix.buckets()
        if "lcp" in tables:
            ix.enable_lcp()
        if docs or freq:
            ix.set_documents(np.array(ts.DOC_OFF, dtype=np.uint32))
        if freq:
            ix.enable_doc_freq()
        self.ix = ix
        return self

    def close(self, abi):
        for kind, h in self.handles:
            getattr(abi.L, kind)(h)
        self.handles.clear()
        for ix in (self.ix, self.tix):
            if ix is not None:
                ix.close()
        self.ix = self.tix = None


class Call:
    """name: the id; fn: the ABI function; kinds: the requests of one successful call, in order; setup(d) -> Ctx (on the pytest
    thread, so the case's thread starts with no read-back block); args(ctx) -> name -> value in the declaration's order, the
    outputs fresh arrays; check(ctx, a, rc): the answers of a successful call are exact; fallbacks: k -> why request k refused is
    no error; probe(ctx, abi): the index under change is as it was; getters: the statistics the call writes; redo: a successful
    call changes the index, so the next one needs a fresh index; after(ctx, a): what a successful call made is the case's"""

    def __init__(self, name, kinds, args, check, setup=None, fallbacks=None, probe=None, getters=(), env=None, redo=False, after=None, fn=None):
        self.name, self.fn, self.kinds, self.args, self.check = name, fn or "sa_amd_" + name, tuple(kinds), args, check
        self.setup, self.fallbacks, self.probe, self.getters = setup or Ctx, dict(fallbacks or {}), probe, tuple(getters)
        self.env, self.redo, self.after = dict(env or {}), redo, after
        assert all(self.kinds[k - 1] in ("pinned", "device", "table") for k in self.fallbacks), name


D, P, Tb = "device", "pinned", "table"
BUILD, LCPS = ("last_stats", "last_host_timing"), ("last_lcp_stats",)


# ---------------------------------------------------------------- the host forms ----

def _saca(text_arr, getters=BUILD):
    def args(c):
        t, _ = text_arr()
        return dict(T=t, SA=out(t.size + 1), n=t.size)
    return args, (lambda c, a, rc: rc == OK and eq(a["SA"], text_arr()[1]))


def _divsufsort_check(c, a, rc):
    return rc == OK and eq(a["SA"].astype(np.uint32), ARR()[1:])


def _spans_args(mode, lead):
    def args(c):
        cap = ts._spans_of("real", mode).shape[0] + 5
        return dict(lead(c), min_len=MIN_LEN, mode=mode, spans=out(2 * cap), capacity=cap, count_out=word())
    return args


def _sub_query():
    return sa.SubstrQuery(ts.SUB_FILTER[0], ts.SUB_FILTER[1], ts.SUB_FILTER[2], ALL, 0)


@functools.lru_cache(maxsize=None)
def _sub_model():
    rows, pos, _ = substrings_model(ts.substrings_ref("real"), ts.SUB_FILTER, ALL, 0)
    return ts._u32(rows), ts._u32(pos)


def _sub_args(lead):
    def args(c):
        cap = _sub_model()[0].shape[0] + 5
        c.extra["q"] = _sub_query()
        return dict(lead(c), query=c.extra["q"], rows=out(_sub_model()[0].shape[1] * cap), pos=out(cap), capacity=cap, total=word())
    return args


def _sub_check(c, a, rc):
    rows, pos = _sub_model()
    k = rows.shape[0]
    return rc == OK and prefix_ok(a["rows"], rows) and prefix_ok(a["pos"], pos) and int(a["total"][0]) == k


@functools.lru_cache(maxsize=None)
def _small():
    return tdb.sais("small_4097")


@functools.lru_cache(maxsize=None)
def _early():
    return tdb.sais("corpus_3m")


@functools.lru_cache(maxsize=None)
def _bwt():
    b, primary = bwt_definition(T(), ARR())
    return np.ascontiguousarray(b), int(primary)


@functools.lru_cache(maxsize=None)
def _packed():
    import pack_model
    small = np.random.default_rng(11).permutation(tdb.SMALL_N).astype(np.uint32)
    return small, np.frombuffer(pack_model.pack(small), dtype=np.uint8).copy()


def _host(c):
    return dict(T=T(), n=N, SA=ARR())


EARLY_ENV = dict(next(env for name, key, env, holds in tdb.BUILDS if name == "early_download"))

HOST_CALLS = [
    Call("saca_u8", (D, P), *_saca(lambda: ts.text("real")), getters=BUILD, fallbacks={1: REDUCED, 2: READBACK}),
    Call("saca_u8-staged", (D, P, P, P, P), *_saca(lambda: ts.text("real")), getters=BUILD, fallbacks={1: REDUCED, 2: READBACK},
         env={"SA_AMD_STAGED_MIN_BYTES": "0"}, fn="sa_amd_saca_u8"),
    Call("saca_u8-early", (D, P, P, P, P), *_saca(_early), getters=BUILD, fallbacks={1: REDUCED, 2: READBACK}, env=EARLY_ENV, fn="sa_amd_saca_u8"),
    Call("saca_u8-small", (P,), *_saca(_small), getters=BUILD, fn="sa_amd_saca_u8"),
    Call("divsufsort", (D, P), lambda c: dict(T=T(), SA=out(N, np.int32), n=N), _divsufsort_check, getters=BUILD, fallbacks={1: REDUCED, 2: READBACK}),
    Call("saca_u8_lcp", (D, P), lambda c: dict(T=T(), SA=out(N + 1), n=N, LCP=out(N + 1)),
         lambda c, a, rc: rc == OK and eq(a["SA"], ARR()) and eq(a["LCP"], ts.lcp_of("real")), getters=LCPS, fallbacks={2: READBACK}),
    Call("lcp", (D, P), lambda c: dict(_host(c), LCP=out(N + 1)), lambda c, a, rc: rc == OK and eq(a["LCP"], ts.lcp_of("real")),
         getters=LCPS, fallbacks={2: READBACK}),
    Call("bucket_table", (D,), lambda c: dict(T=T(), n=N, SA=None, bkt=out(65793)),
         lambda c, a, rc: rc == OK and eq(a["bkt"], tdb.oracle().bucket_table(T()))),
    Call("saca_u8_buckets", (Tb, Tb, Tb, Tb, P), lambda c: dict(T=T(), SA=out(N + 1), n=N, bkt=out(65793)),
         lambda c, a, rc: rc == OK and eq(a["SA"], ARR()) and eq(a["bkt"], tdb.oracle().bucket_table(T())), fallbacks={5: READBACK}),
    Call("check_integrity", (Tb, Tb, Tb, P), lambda c: dict(_host(c), sa_len=N + 1), lambda c, a, rc: rc == 1, fallbacks={3: SMALLER, 4: READBACK}),
    Call("check_integrity-wrong", (Tb, Tb, Tb, P), lambda c: dict(T=T(), n=N, SA=ts.text("decoy")[1], sa_len=N + 1), lambda c, a, rc: rc == 0,
         fallbacks={3: SMALLER, 4: READBACK}, fn="sa_amd_check_integrity"),
    Call("pack", (Tb, Tb), lambda c: dict(SA=_packed()[0], length=tdb.SMALL_N, out=out(sa.lib().sa_amd_pack_bound(tdb.SMALL_N), np.uint8),
                                           capacity=sa.lib().sa_amd_pack_bound(tdb.SMALL_N), out_len=word()),
         lambda c, a, rc: rc == OK and int(a["out_len"][0]) == _packed()[1].size and eq(a["out"][:_packed()[1].size], _packed()[1])),
         # (behind out_len the call may have written: the trimmed zero bytes of the last block lie inside sa_amd_pack_bound)
    Call("unpack", (Tb, Tb), lambda c: dict(bytes=_packed()[1], nbytes=_packed()[1].size, SA=out(tdb.SMALL_N), capacity=tdb.SMALL_N, length=word()),
         lambda c, a, rc: rc == OK and int(a["length"][0]) == tdb.SMALL_N and eq(a["SA"], _packed()[0])),
    Call("bwt", (D, P), lambda c: dict(_host(c), BWT=out(N, np.uint8), primary_out=word(np.int32)),
         lambda c, a, rc: rc == OK and eq(a["BWT"], _bwt()[0]) and int(a["primary_out"][0]) == _bwt()[1], fallbacks={2: READBACK}),
    Call("bwt-built", (D, P), lambda c: dict(T=T(), n=N, SA=None, BWT=out(N, np.uint8), primary_out=word(np.int32)),
         lambda c, a, rc: rc == OK and eq(a["BWT"], _bwt()[0]) and int(a["primary_out"][0]) == _bwt()[1], fallbacks={2: READBACK}, fn="sa_amd_bwt"),
    Call("unbwt", (D, P), lambda c: dict(BWT=_bwt()[0], n=N, primary=_bwt()[1], T_out=out(N, np.uint8)),
         lambda c, a, rc: rc == OK and eq(a["T_out"], T()), getters=("last_unbwt_stats",), fallbacks={2: READBACK}),
    Call("repeat_lengths", (D, P), lambda c: dict(_host(c), LR=out(N)), lambda c, a, rc: rc == OK and eq(a["LR"], ts._u32(ts.lr_of("real"))),
         getters=("last_repeat_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("repeat_spans", (D, P), _spans_args(sa.REPEATS_KEEP_FIRST, _host),
         lambda c, a, rc: rc == OK and rows_ok(a["spans"], ts._spans_of("real", sa.REPEATS_KEEP_FIRST), a["count_out"]),
         getters=("last_repeat_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("lpf", (D, P), lambda c: dict(_host(c), LPF=out(N), SRC=out(N)),
         lambda c, a, rc: rc == OK and eq(a["LPF"], ts._u32(ts.lpf_of("real")[0])) and eq(a["SRC"], ts._u32(ts.lpf_of("real")[1])),
         getters=("last_lz_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("lz77", (D, P), lambda c: dict(_host(c), phrases=out(2 * (_phrases().shape[0] + 5)), capacity=_phrases().shape[0] + 5, count_out=word()),
         lambda c, a, rc: rc == OK and rows_ok(a["phrases"], _phrases(), a["count_out"]), getters=("last_lz_stats", "last_lcp_stats"),
         fallbacks={2: READBACK}),
    Call("substrings", (D, P), _sub_args(_host), _sub_check, getters=("last_substr_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
]


@functools.lru_cache(maxsize=None)
def _phrases():
    return ts._u32(parse_definition(*ts.lpf_of("real")))


# ---------------------------------------------------------------- the index forms ----

def _ix(c):
    return dict(ix=c.ix)


def plain(d):
    return Ctx(d).index()


def with_tables(d):
    return Ctx(d).index(("bkt", "lcp"))


def with_docs(d):
    return Ctx(d).index(docs=True)


def with_freq(d):
    return Ctx(d).index(freq=True)


def _index_answers(abi, h):
    """the array an index handle holds"""
    got = out(N + 1)
    assert abi.L.sa_amd_index_sa(h, got.ctypes.data) == OK
    return got


def _created(kind_destroy, reader, want):
    """check and after of a creating call: the handle is no canary, the index holds the reference array; it is the case's to destroy"""
    def check(c, a, rc):
        h = int(a["out"][0])
        if rc != OK or h == 0 or ra.untouched(a["out"]):
            return False
        c.handles.append((kind_destroy, h))
        got = out(want().size)
        return getattr(c.extra["abi"].L, reader)(h, got.ctypes.data) == OK and eq(got, want())
    return check


@functools.lru_cache(maxsize=None)
def _search_patterns():
    pats, want, _ = tdb._search_case()
    return ra.pattern_batch(pats), want


def _search_args(c):
    (data, off, cnt), _ = _search_patterns()
    return dict(_ix(c), pat_data=data, pat_off=off, count=cnt, contains=out(cnt, np.uint8), range_lo=out(cnt), range_hi=out(cnt), lcp_start=out(cnt),
                lcp_len=out(cnt))


def _search_check(c, a, rc):
    _, want = _search_patterns()
    ok = rc == OK
    for q, (lo, hi) in enumerate(want):
        ok = ok and bool(a["contains"][q]) == (hi > lo) and int(a["range_hi"][q]) - int(a["range_lo"][q]) == hi - lo
        ok = ok and (hi == lo or int(a["range_lo"][q]) == lo)
    return ok


def _probe_search(c, abi):
    """the index answers the searches as before (whatever tables it had: the answers do not depend on them)"""
    a = _search_args(c)
    return abi.call("sa_amd_index_search", a) == OK and _search_check(c, a, OK)


def _match_args(c):
    return dict(_ix(c), Q=ts.query("real"), m=ts.M, max_len=1 << 20, ML=out(ts.M), POS=out(ts.M))


def _match_spans_args(c):
    cap = ts._match_spans("real").shape[0] + 5
    return dict(_ix(c), Q=ts.query("real"), m=ts.M, min_len=MIN_LEN, spans=out(2 * cap), capacity=cap, count_out=word())


INDEX_CALLS = [
    Call("index_create", (Tb, Tb), lambda c: dict(T=T(), n=N, SA=ARR(), out=word(np.uint64)), _created("sa_amd_index_destroy", "sa_amd_index_sa", ARR)),
    Call("index_create-built", (Tb, Tb, Tb, P), lambda c: dict(T=T(), n=N, SA=None, out=word(np.uint64)),
         _created("sa_amd_index_destroy", "sa_amd_index_sa", ARR), fallbacks={4: READBACK}, fn="sa_amd_index_create"),
    Call("index_destroy", (), lambda c: dict(ix=c.extra["h"]), lambda c, a, rc: True,
         setup=lambda d: Ctx(d)),                                     # (the handle is made on the case's thread: see _destroy_args)
    Call("index_sa", (), lambda c: dict(_ix(c), SA_out=out(N + 1)), lambda c, a, rc: rc == OK and eq(a["SA_out"], ARR()), setup=plain),
    Call("index_buckets", (Tb,), lambda c: dict(_ix(c), bkt=out(65793)), lambda c, a, rc: rc == OK and eq(a["bkt"], tdb.oracle().bucket_table(T())),
         setup=plain, probe=_probe_search, redo=True),
    Call("index_check_integrity", (D, P), _ix, lambda c, a, rc: rc == 1, setup=plain, fallbacks={1: SMALLER, 2: READBACK}),
    Call("index_search", (Tb, Tb, Tb, Tb, Tb), _search_args, _search_check, setup=with_tables, getters=("last_search_stats",)),
    Call("index_lcp", (D, P), lambda c: dict(_ix(c), LCP=out(N + 1)), lambda c, a, rc: rc == OK and eq(a["LCP"], ts.lcp_of("real")), setup=plain,
         getters=LCPS, fallbacks={2: READBACK}),
    Call("index_enable_lcp", (Tb, D, P), _ix, lambda c, a, rc: rc == OK and _probe_search(c, c.extra["abi"]), setup=plain, probe=_probe_search,
         getters=LCPS, fallbacks={3: READBACK}, redo=True),
    Call("index_bwt", (D, P), lambda c: dict(_ix(c), BWT=out(N, np.uint8), primary_out=word(np.int32)),
         lambda c, a, rc: rc == OK and eq(a["BWT"], _bwt()[0]) and int(a["primary_out"][0]) == _bwt()[1], setup=plain, fallbacks={2: READBACK}),
    Call("index_repeat_lengths", (D, P), lambda c: dict(_ix(c), LR=out(N)), lambda c, a, rc: rc == OK and eq(a["LR"], ts._u32(ts.lr_of("real"))),
         setup=plain, getters=("last_repeat_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("index_repeat_spans", (D, P), _spans_args(sa.REPEATS_ALL, _ix),
         lambda c, a, rc: rc == OK and rows_ok(a["spans"], ts._spans_of("real", sa.REPEATS_ALL), a["count_out"]), setup=plain,
         getters=("last_repeat_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("index_lpf", (D, P), lambda c: dict(_ix(c), LPF=out(N), SRC=out(N)),
         lambda c, a, rc: rc == OK and eq(a["LPF"], ts._u32(ts.lpf_of("real")[0])) and eq(a["SRC"], ts._u32(ts.lpf_of("real")[1])), setup=plain,
         getters=("last_lz_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("index_lz77", (D, P), lambda c: dict(_ix(c), phrases=out(2 * (_phrases().shape[0] + 5)), capacity=_phrases().shape[0] + 5, count_out=word()),
         lambda c, a, rc: rc == OK and rows_ok(a["phrases"], _phrases(), a["count_out"]), setup=plain, getters=("last_lz_stats", "last_lcp_stats"),
         fallbacks={2: READBACK}),
    Call("index_substrings", (D, P), _sub_args(_ix), _sub_check, setup=plain, getters=("last_substr_stats", "last_lcp_stats"), fallbacks={2: READBACK}),
    Call("index_match_stats", (D, P), _match_args,
         lambda c, a, rc: rc == OK and eq(a["ML"], ts._u32(ts._match("real")[0])) and eq(a["POS"], ts._u32(ts._match("real")[1])), setup=with_tables,
         getters=("last_match_stats",), fallbacks={2: READBACK}),
    Call("index_match_spans", (D, P), _match_spans_args, lambda c, a, rc: rc == OK and rows_ok(a["spans"], ts._match_spans("real"), a["count_out"]),
         setup=plain, getters=("last_match_stats",), fallbacks={2: READBACK}),
]


def _destroy_args(c):
    """sa_amd_index_destroy: the index it frees is made by the call before it, on the same thread, outside the count"""
    h = ctypes.c_void_p()
    assert sa.lib().sa_amd_index_create(T().ctypes.data, N, ARR().ctypes.data, ctypes.byref(h)) == OK
    return dict(ix=h.value)


INDEX_CALLS[2].args = _destroy_args


# ---------------------------------------------------------------- documents ----

OFF_B = tuple(ts.DOC_OFF[::2]) + ((N,) if ts.DOC_OFF[::2][-1] != N else ())      # another collection: every second boundary


@functools.lru_cache(maxsize=None)
def _doc_answers(off=ts.DOC_OFF):
    return docs_answers_definition(TB(), off, ARR(), tdb._doc_patterns())


@functools.lru_cache(maxsize=None)
def _doc_batch():
    return ra.pattern_batch(tdb._doc_patterns())


def _docs_lead(c):
    data, off, cnt = _doc_batch()
    return dict(_ix(c), pat_data=data, pat_off=off, count=cnt)


def _doc_search_check(c, a, rc, off=ts.DOC_OFF):
    occ, df, _ = _doc_answers(off)
    return rc == OK and eq(a["occ"], ts._u32(occ)) and eq(a["df"], ts._u32(df))


def _probe_docs(off, freq):
    def probe(c, abi):
        """the collection `off` still answers doc_search; with `freq`, doc_tf still works"""
        a = dict(_docs_lead(c), occ=out(_doc_batch()[2]), df=out(_doc_batch()[2]))
        ok = abi.call("sa_amd_index_doc_search", a) == OK and _doc_search_check(c, a, OK, off)
        if freq:
            b = _tf_args(c)
            ra.fill_canary(abi.outputs("sa_amd_index_doc_tf", b))
            ok = ok and abi.call("sa_amd_index_doc_tf", b) == OK and _tf_check(c, b, OK)
        return ok
    return probe


def _listing_of(lists):
    loff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return loff, ts._u32(np.concatenate(list(lists) + [np.zeros(0, dtype=np.int64)]))


def _doc_list_args(c):
    total = int(_doc_answers()[1].sum())
    return dict(_docs_lead(c), list_off=out(_doc_batch()[2] + 1, np.int64), docs=out(total + 5), capacity=total + 5, total_out=word())


def _doc_list_check(c, a, rc):
    loff, docs = _listing_of(_doc_answers()[2])
    return rc == OK and eq(a["list_off"], loff) and eq(a["docs"][:docs.size], docs) and ra.untouched(a["docs"][docs.size:]) \
        and int(a["total_out"][0]) == docs.size


def _tf_args(c):
    total = sum(len(ls) for _, ls, _ in tdb._tf_answers())
    return dict(_docs_lead(c), list_off=out(_doc_batch()[2] + 1, np.int64), docs=out(total + 5), tf=out(total + 5), capacity=total + 5, total_out=word())


def _tf_check(c, a, rc):
    ans = tdb._tf_answers()
    loff, docs = _listing_of([ls for _, ls, _ in ans])
    _, tf = _listing_of([t for _, _, t in ans])
    return rc == OK and eq(a["list_off"], loff) and eq(a["docs"][:docs.size], docs) and eq(a["tf"][:tf.size], tf) and int(a["total_out"][0]) == docs.size \
        and ra.untouched(a["docs"][docs.size:]) and ra.untouched(a["tf"][tf.size:])


TOPK = 5


def _topk_args(c):
    cnt = _doc_batch()[2]
    return dict(_docs_lead(c), k=TOPK, top_off=out(cnt + 1, np.int64), docs=out(cnt * TOPK), tf=out(cnt * TOPK))


def _topk_check(c, a, rc):
    tops = [topk_definition(ls, t, TOPK) for _, ls, t in tdb._tf_answers()]
    loff, docs = _listing_of([d for d, _ in tops])
    _, tf = _listing_of([t for _, t in tops])
    return rc == OK and eq(a["top_off"], loff) and eq(a["docs"][:docs.size], docs) and eq(a["tf"][:tf.size], tf) \
        and ra.untouched(a["docs"][docs.size:]) and ra.untouched(a["tf"][tf.size:])


@functools.lru_cache(maxsize=None)
def _doc_repeats():
    r = doc_repeats_definition(T(), ts.DOC_OFF, ARR(), tdb._doc_repeat_lcp(), MIN_LEN, sa.REPEATS_ALL, sa.DOCREP_OTHER)
    return ts._u32(r["spans"]), ts._u32(r["doc_bytes"])


def _doc_repeat_args(c):
    cap = _doc_repeats()[0].shape[0] + 5
    return dict(_ix(c), min_len=MIN_LEN, mode=sa.REPEATS_ALL, scope=sa.DOCREP_OTHER, spans=out(2 * cap), capacity=cap, count_out=word(),
                doc_bytes=out(len(ts.DOC_OFF) - 1))


@functools.lru_cache(maxsize=None)
def _dsub_model():
    rows, df, pos, _ = doc_substrings_model(ts.substrings_ref("real"), "dirty", ts.DOC_OFF, ts.SUB_FILTER, 2, ALL, 0)
    return ts._u32(rows), ts._u32(df), ts._u32(pos)


def _dsub_args(c):
    cap = _dsub_model()[0].shape[0] + 5
    c.extra["q"] = sa.DocSubstrQuery(ts.SUB_FILTER[0], ts.SUB_FILTER[1], ts.SUB_FILTER[2], ALL, 0, 2)
    return dict(_ix(c), query=c.extra["q"], rows=out(_dsub_model()[0].shape[1] * cap), df=out(cap), pos=out(cap), capacity=cap, total=word())


def _dsub_check(c, a, rc):
    rows, df, pos = _dsub_model()
    k = rows.shape[0]
    return rc == OK and prefix_ok(a["rows"], rows) and prefix_ok(a["df"], df) and prefix_ok(a["pos"], pos) and int(a["total"][0]) == k


def _set_documents_check(c, a, rc):
    """the new collection answers (through the wrapper's own check, told of the new collection)"""
    if rc != OK:
        return False
    c.ix._ndocs = len(OFF_B) - 1
    check_queries(c.ix, TB(), OFF_B, ARR(), tdb._doc_patterns(), chunk=tdb.DOC_CHUNK)
    return True


@functools.lru_cache(maxsize=None)
def _positions():
    return np.ascontiguousarray(ts.positions("real"))


DOC_CALLS = [
    Call("index_set_documents", (Tb, Tb, D, P), lambda c: dict(_ix(c), doc_off=np.array(OFF_B, dtype=np.uint32), ndocs=len(OFF_B) - 1),
         _set_documents_check, setup=with_freq, probe=_probe_docs(ts.DOC_OFF, True), fallbacks={4: READBACK}, redo=True),
    Call("index_doc_of", (D,), lambda c: dict(_ix(c), pos=_positions(), count=ts.POS_COUNT, doc_out=out(ts.POS_COUNT)),
         lambda c, a, rc: rc == OK and eq(a["doc_out"], ts._u32(doc_of_definition(ts.DOC_OFF, N, _positions()))), setup=with_docs),
    Call("index_doc_search", (D, P), lambda c: dict(_docs_lead(c), occ=out(_doc_batch()[2]), df=out(_doc_batch()[2])), _doc_search_check,
         setup=with_docs, getters=("last_docs_stats",), fallbacks={2: READBACK}),
    Call("index_doc_list", (D, P, D), _doc_list_args, _doc_list_check, setup=with_docs, getters=("last_docs_stats",), fallbacks={2: READBACK}),
    Call("index_doc_repeat_spans", (D, P), _doc_repeat_args,
         lambda c, a, rc: rc == OK and rows_ok(a["spans"], _doc_repeats()[0], a["count_out"]) and eq(a["doc_bytes"], _doc_repeats()[1]),
         setup=with_docs, getters=("last_doc_repeat_stats", "last_repeat_stats"), fallbacks={2: READBACK}),
    Call("index_enable_doc_freq", (Tb, D, P), _ix, lambda c, a, rc: rc == OK and _probe_docs(ts.DOC_OFF, True)(c, c.extra["abi"]), setup=with_docs,
         probe=_probe_docs(ts.DOC_OFF, False), fallbacks={3: READBACK}, redo=True),
    Call("index_doc_tf", (D, P, D, D), _tf_args, _tf_check, setup=with_freq, getters=("last_doc_tf_stats",), fallbacks={2: READBACK}),
    Call("index_doc_topk", (D, P, D, D), _topk_args, _topk_check, setup=with_freq, getters=("last_doc_tf_stats",), fallbacks={2: READBACK}),
    Call("index_doc_substrings", (D, P), _dsub_args, _dsub_check, setup=with_docs, getters=("last_doc_substr_stats",), fallbacks={2: READBACK}),
]


# ---------------------------------------------------------------- the n-gram queries and the score ----

def _ngram_args(backoff):
    def args(c):
        ctx, exp, prompts = tdb._ngram_case()
        pats = prompts if backoff else ctx
        data, off, cnt = ra.pattern_batch(pats)
        cap = 256 * cnt
        a = dict(_ix(c), pat_data=data, pat_off=off, count=cnt)
        if backoff:
            a.update(min_count=2, max_len=0, suffix_len=out(cnt))
        a.update(range_lo=out(cnt), range_hi=out(cnt), at_end=out(cnt, np.uint8), list_off=out(cnt + 1, np.int64), bytes=out(cap, np.uint8),
                 counts=out(cap), capacity=cap, total_out=word())
        return a
    return args


@functools.lru_cache(maxsize=None)
def _infgram_defs():
    return [infgram_definition(TB(), ARR(), p, 2, 0) for p in tdb._ngram_case()[2]]


def _ngram_check(backoff):
    def check(c, a, rc):
        if rc != OK:
            return False
        exp = [d[1:5] for d in _infgram_defs()] if backoff else tdb._ngram_case()[1]
        total = int(a["total_out"][0])
        got = {"total": total, "lo": a["range_lo"], "hi": a["range_hi"], "at_end": a["at_end"], "list_off": a["list_off"], "bytes": a["bytes"][:total],
               "counts": a["counts"][:total]}
        check_ngram_outputs(got, exp, c.extra.get("what"))
        return (not backoff or eq(a["suffix_len"], ts._u32([d[0] for d in _infgram_defs()]))) and ra.untouched(a["bytes"][total:]) \
            and ra.untouched(a["counts"][total:])
    return check


def _score_args(c):
    a = dict(_ix(c), Q=ts.query("real"), m=ts.M, q_off=np.array(ts.Q_OFF, dtype=np.int64), ndocs=len(ts.Q_OFF) - 1, min_count=1, max_len=sa.SCORE_MAX_CONTEXT)
    a.update({k: out(ts.M, np.uint8 if k == "AT_END" else np.uint32) for k in ("S", "LO", "HI", "AT_END", "NLO", "NHI")})
    return a


def _score_check(c, a, rc):
    want = ts._score("real")
    return rc == OK and all(eq(a[k.upper()].astype(np.int64), want[k].astype(np.int64)) for k in ts.SCORE_NAMES)


NGRAM_CALLS = [
    Call("index_next_bytes", (D, P), _ngram_args(False), _ngram_check(False), setup=plain, getters=("last_ngram_stats",), fallbacks={2: READBACK}),
    Call("index_infgram", (D, P), _ngram_args(True), _ngram_check(True), setup=plain, getters=("last_ngram_stats",), fallbacks={2: READBACK}),
    Call("index_infgram_score", (D, P), _score_args, _score_check, setup=with_tables, getters=("last_score_stats",), fallbacks={2: READBACK}),
]


# ---------------------------------------------------------------- the token texts, 16 and 32 bits ----

@functools.lru_cache(maxsize=None)
def _token_case32():
    """test_tokens32's index text without its indexes"""
    m = tk32.Model.__new__(tk32.Model)
    planted = np.empty(1200, dtype=np.uint32)
    planted[0::2] = tk32.HOT
    planted[1::2] = 1000 + np.arange(600) % 300 + (np.arange(600) // 300) * 0x010000
    body = corpus.token_corpus_u32(6000, 200000, 9)
    m.tok = np.ascontiguousarray(np.concatenate((body[:3000], planted, body[3000:])), dtype=np.uint32)
    m.tok.setflags(write=False)
    m.t = [int(x) for x in m.tok]
    m.n = len(m.t)
    m.arr = reference_suffix_array32(m.tok, tdb.oracle())
    m.lst = m.arr.tolist()
    pats, ctx, prompts = tk32._search_patterns(m), tk32._contexts(m), tk32._prompts(m)
    return m, pats, [tok_range_definition(m.t, m.lst, p) for p in pats], ctx, [next_tokens_definition(m.t, m.lst, c) for c in ctx], \
        prompts, [tok_infgram_definition(m.t, m.lst, p, 2, 0) for p in prompts]


class Tokens:
    """the functions of one token width: the case of the text, the dtype, the prefix of the ABI names, the wrapper's index type"""

    def __init__(self, case, dtype, prefix, saca, index_type, limit):
        self.case, self.dtype, self.prefix, self.saca, self.index_type, self.limit = case, dtype, prefix, saca, index_type, limit

    def setup(self, d):
        c = Ctx(d)
        m = self.case()[0]
        c.tix = self.index_type(m.tok, np.array(m.arr, dtype=np.uint32))
        c.d._made.append(c.tix)
        return c

    def lead(self, c, pats):
        data, off, cnt = ra.pattern_batch(pats, self.dtype)
        return dict(ix=c.tix, pat_data=data, pat_off=off, count=cnt)

    def search_args(self, c):
        a = self.lead(c, self.case()[1])
        cnt = a["count"]
        return dict(a, contains=out(cnt, np.uint8), range_lo=out(cnt), range_hi=out(cnt))

    def search_check(self, c, a, rc):
        want = self.case()[2]
        return rc == OK and [(int(x), int(y)) for x, y in zip(a["range_lo"], a["range_hi"])] == want \
            and [bool(x) for x in a["contains"]] == [hi > lo for lo, hi in want]

    def query_args(self, backoff):
        def args(c):
            case = self.case()
            a = self.lead(c, case[5] if backoff else case[3])
            cnt = a["count"]
            cap = sum(len(w[-1]) for w in (case[6] if backoff else case[4])) + 5
            if backoff:
                a.update(min_count=2, max_len=0, suffix_len=out(cnt))
            a.update(range_lo=out(cnt), range_hi=out(cnt), at_end=out(cnt, np.uint8), list_off=out(cnt + 1, np.int64), tokens=out(cap, self.dtype),
                     counts=out(cap), capacity=cap, total_out=word())
            return a
        return args

    def query_check(self, backoff):
        def check(c, a, rc):
            want = self.case()[6 if backoff else 4]
            ok = rc == OK
            for q, w in enumerate(want):
                ws = w[0] if backoff else None
                wlo, whi, wae, wl = w[1:] if backoff else w
                ok = ok and (int(a["range_lo"][q]), int(a["range_hi"][q]), int(a["at_end"][q])) == (wlo, whi, wae)
                ok = ok and tk._listing(a["list_off"], a["tokens"], a["counts"], q) == wl and (not backoff or int(a["suffix_len"][q]) == ws)
            total = int(a["total_out"][0])
            return ok and total == int(a["list_off"][-1]) and ra.untouched(a["tokens"][total:]) and ra.untouched(a["counts"][total:])
        return check

    def calls(self, score_args, score_check, score_setup):
        p, m = self.prefix, lambda: self.case()[0]
        destroy, reader = "sa_amd_%s_destroy" % p, "sa_amd_%s_sa" % p
        return [
            Call(self.saca, (D, P), lambda c: dict(T=m().tok, SA=out(m().n + 1), n=m().n), lambda c, a, rc: rc == OK and eq(a["SA"], m().arr),
                 fallbacks={2: READBACK}),
            Call(p + "_create", (Tb, Tb, D, P), lambda c: dict(T=m().tok, n=m().n, SA=np.array(m().arr, dtype=np.uint32), out=word(np.uint64)),
                 _created(destroy, reader, lambda: np.asarray(m().arr, dtype=np.uint32)), fallbacks={4: READBACK}),
            Call(p + "_create-built", (Tb, Tb, D, P), lambda c: dict(T=m().tok, n=m().n, SA=None, out=word(np.uint64)),
                 _created(destroy, reader, lambda: np.asarray(m().arr, dtype=np.uint32)), fallbacks={4: READBACK}, fn="sa_amd_%s_create" % p),
            Call(p + "_sa", (), lambda c: dict(ix=c.tix, SA_out=out(m().n + 1)), lambda c, a, rc: rc == OK and eq(a["SA_out"], m().arr), setup=self.setup),
            Call(p + "_search", (D,), self.search_args, self.search_check, setup=self.setup),
            Call(p + "_next_tokens", (D, P, D), self.query_args(False), self.query_check(False), setup=self.setup, getters=("last_tok_stats",),
                 fallbacks={2: READBACK}),
            Call(p + "_infgram", (D, P, D), self.query_args(True), self.query_check(True), setup=self.setup, getters=("last_tok_stats",),
                 fallbacks={2: READBACK}),
            Call(p + "_infgram_score", (D, P), score_args, score_check, setup=score_setup, getters=("last_tok_score_stats",), fallbacks={2: READBACK}),
        ]


TOK16 = Tokens(tdb._token_case, np.uint16, "tok_index", "saca_u16", sa.TokenIndex, 1 << 16)
TOK32 = Tokens(_token_case32, np.uint32, "tok32_index", "saca_u32", sa.TokenIndex32, 1 << 24)
SCORE_OUTS = ("S", "LO", "HI", "AT_END", "NLO", "NHI")


def _tok_score_setup(d):
    c = Ctx(d)
    Tz = token_text("zipf")
    c.tix = d.token_index(Tz.tok, np.array(Tz.arr, dtype=np.uint32))
    return c


def _tok_score_args(c):
    q, off = composite_query(token_text("zipf"))
    a = dict(ix=c.tix, Q=q, m=q.size, q_off=np.ascontiguousarray(off, dtype=np.int64), ndocs=len(off) - 1, min_count=1, max_len=sa.SCORE_MAX_CONTEXT)
    a.update({k: out(q.size, np.uint8 if k == "AT_END" else np.uint32) for k in SCORE_OUTS})
    return a


def _tok_score_check(c, a, rc):
    Tz = token_text("zipf")
    q, off = composite_query(Tz)
    d = tok_score_definition(Tz, q, off, 1, sa.SCORE_MAX_CONTEXT)
    return rc == OK and all(eq(a[k.upper()].astype(np.int64), np.asarray(d[k]).astype(np.int64)) for k in ts.SCORE_NAMES)


@functools.lru_cache(maxsize=None)
def _tok32_query():
    """a short scored query of the 32-bit text: two documents, a slice of the text and one with an id the text does not hold"""
    m = _token_case32()[0]
    q = np.array(m.t[100:148] + [tk32.HOT, 999] + m.t[m.n - 14:], dtype=np.uint32)
    off = np.array([0, 48, q.size], dtype=np.int64)
    d = tok_score_definition_lists(m.t, m.lst, [int(x) for x in q], off, 1, sa.SCORE_MAX_CONTEXT)
    return q, off, d


def _tok32_score_args(c):
    q, off, _ = _tok32_query()
    a = dict(ix=c.tix, Q=q, m=q.size, q_off=off, ndocs=len(off) - 1, min_count=1, max_len=sa.SCORE_MAX_CONTEXT)
    a.update({k: out(q.size, np.uint8 if k == "AT_END" else np.uint32) for k in SCORE_OUTS})
    return a


def _tok32_score_check(c, a, rc):
    d = _tok32_query()[2]
    return rc == OK and all(eq(a[k.upper()].astype(np.int64), np.asarray(d[k]).astype(np.int64)) for k in ts.SCORE_NAMES)


TOKEN_CALLS = TOK16.calls(_tok_score_args, _tok_score_check, _tok_score_setup) + TOK32.calls(_tok32_score_args, _tok32_score_check, TOK32.setup)


# ---------------------------------------------------------------- Boolean document queries ----

@functools.lru_cache(maxsize=None)
def _dm_case():
    """three queries over the patterns of the document cases: AND, OR inside a clause, NOT"""
    pats = [p for p in tdb._doc_patterns() if p][:6]
    queries = [[pats[0], pats[1]], [[pats[2], pats[3]], sa.Not(pats[4])], [pats[5]]]
    return queries, sa._query_batch(queries), doc_match_definition(TB(), ts.DOC_OFF, ARR(), queries)


def _dm_lead(c):
    pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries = _dm_case()[1]
    sa.doc_match_set_budget(BUDGET_MIN)                               # (per thread: several slabs share the one block)
    return dict(_ix(c), pat_data=np.ascontiguousarray(pat_data), pat_off=np.ascontiguousarray(pat_off, dtype=np.int64), npat=npat,
                clause_off=np.ascontiguousarray(clause_off, dtype=np.int32), clause_flags=np.ascontiguousarray(clause_flags, dtype=np.uint8),
                nclauses=nclauses, query_off=np.ascontiguousarray(query_off, dtype=np.int32), nqueries=nqueries)


def _dm_check(c, a, rc):
    df, cdf, _ = _dm_case()[2]
    return rc == OK and eq(a["df"], ts._u32(df)) and eq(a["clause_df"], ts._u32(cdf))


def _dm_list_args(c):
    total = int(_dm_case()[2][0].sum())
    return dict(_dm_lead(c), list_off=out(_dm_case()[1][7] + 1, np.int64), docs=out(total + 5), capacity=total + 5, total_out=word())


def _dm_list_check(c, a, rc):
    loff, docs = _listing_of(_dm_case()[2][2])
    return rc == OK and eq(a["list_off"], loff) and eq(a["docs"][:docs.size], docs) and ra.untouched(a["docs"][docs.size:]) \
        and int(a["total_out"][0]) == docs.size


DOC_MATCH_CALLS = [
    Call("index_doc_match", (D, P, D), lambda c: dict(_dm_lead(c), df=out(_dm_case()[1][7]), clause_df=out(_dm_case()[1][5])), _dm_check, setup=with_docs,
         fallbacks={2: READBACK}),
    Call("index_doc_match_list", (D, P, D), _dm_list_args, _dm_list_check, setup=with_docs, fallbacks={2: READBACK}),
]


# ---------------------------------------------------------------- the *_device forms: one per family ----
# They work in the caller's block: what they request themselves is the thread's pinned read-back block at the most.

class DeviceBuffers:
    def __init__(self):
        self.hip, self.all = ts._hip(), []

    def take(self, size, data=None):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(int(size), 1)) == 0
        self.all.append(p.value)
        if data is None:
            assert self.hip.hipMemset(p.value, ts.CANARY, int(size)) == 0
        else:
            assert self.hip.hipMemcpy(p.value, np.ascontiguousarray(data).ctypes.data, int(size), ts.H2D) == 0
        return p.value

    def read(self, p, count, dtype=np.uint32):
        got = np.zeros(count, dtype=dtype)
        assert self.hip.hipMemcpy(got.ctypes.data, p, got.nbytes, ts.D2H) == 0
        return got

    def free(self):
        for p in self.all:
            self.hip.hipFree(p)
        self.all.clear()


def _device_setup(index):
    def setup(d):
        c = Ctx(d).index() if index else Ctx(d)
        c.extra["dev"] = DeviceBuffers()
        return c
    return setup


def _saca_device_args(c):
    b = c.extra["dev"]
    wb = sa.workspace_bytes(N)
    c.extra["out"] = b.take(4 * (N + 1))
    return dict(dT=b.take(N + 16, np.concatenate([T(), np.zeros(16, np.uint8)])), dSA=c.extra["out"], n=N, dWork=b.take(wb), work_bytes=wb, stream=None,
                stats=None)


def _lcp_device_args(c):
    b = c.extra["dev"]
    wb = sa.lcp_work_bytes(N)
    c.extra["out"] = b.take(4 * (N + 1))
    return dict(dT=b.take(N + 16, np.concatenate([T(), np.zeros(16, np.uint8)])), dSA=b.take(4 * (N + 1), ARR()), n=N, dLCP=c.extra["out"],
                dWork=b.take(wb), work_bytes=wb, stream=None)


def _match_device_args(c):
    b = c.extra["dev"]
    wb = sa.match_work_bytes(ts.M)
    c.extra["out"] = (b.take(4 * ts.M), b.take(4 * ts.M))
    return dict(_ix(c), dQ=b.take(ts.M + 16, np.concatenate([ts.query("real"), np.zeros(16, np.uint8)])), m=ts.M, max_len=1 << 20, dML=c.extra["out"][0],
                dPOS=c.extra["out"][1], dWork=b.take(wb), work_bytes=wb, stream=None)


DEVICE_CALLS = [
    Call("saca_device", (P,), _saca_device_args, lambda c, a, rc: rc == OK and eq(c.extra["dev"].read(c.extra["out"], N + 1), ARR()),
         setup=_device_setup(False), getters=("last_stats",), fallbacks={1: READBACK}),
    Call("lcp_device", (P,), _lcp_device_args, lambda c, a, rc: rc == OK and eq(c.extra["dev"].read(c.extra["out"], N + 1), ts.lcp_of("real")),
         setup=_device_setup(False), getters=LCPS, fallbacks={1: READBACK}),
    Call("index_match_stats_device", (P,), _match_device_args,
         lambda c, a, rc: rc == OK and eq(c.extra["dev"].read(c.extra["out"][0], ts.M), ts._u32(ts._match("real")[0]))
         and eq(c.extra["dev"].read(c.extra["out"][1], ts.M), ts._u32(ts._match("real")[1])),
         setup=_device_setup(True), getters=("last_match_stats",), fallbacks={1: READBACK}),
]

CALLS = HOST_CALLS + INDEX_CALLS + DOC_CALLS + NGRAM_CALLS + TOKEN_CALLS + DOC_MATCH_CALLS + DEVICE_CALLS
BY_NAME = {c.name: c for c in CALLS}
FALLBACKS = {(c.name, c.kinds[k - 1], k): why for c in CALLS for k, why in c.fallbacks.items()}

# every other function of the headers: why it has no refused-allocation case
NO_CASE = {fn: why for fn, why in tdb.NO_CASE.items() if why.startswith(("a getter", "a setter", "a size query", "no device work"))}
NO_CASE["sa_amd_last_doc_match_stats"] = "a getter: it reads what a call left for its thread"
NO_CASE["sa_amd_saca_batch"] = ("every request is made by its worker threads (std::thread per device), out of reach of a per-thread switch: the calling "
                                "thread requests nothing.  No process-wide mode is built for it; the workers run build_host and the small-batch route, "
                                "whose requests the saca_u8 cases refuse one by one")
ONE_PER_FAMILY = "works in the caller's block; one *_device form per family has a case: "
NO_CASE.update({fn: ONE_PER_FAMILY + "sa_amd_lcp_device (the derived arrays share read_words as their only request)" for fn in (
    "sa_amd_bwt_device", "sa_amd_unbwt_device", "sa_amd_repeat_lengths_device", "sa_amd_repeat_spans_device", "sa_amd_lpf_device", "sa_amd_lz77_device",
    "sa_amd_substrings_device", "sa_amd_bucket_table_device", "sa_amd_check_integrity_device")})
NO_CASE.update({fn: ONE_PER_FAMILY + "sa_amd_index_match_stats_device" for fn in (
    "sa_amd_index_match_spans_device", "sa_amd_index_doc_of_device", "sa_amd_index_infgram_score_device")})
NO_CASE["sa_amd_tok_index_destroy"] = NO_CASE["sa_amd_tok32_index_destroy"] = \
    "frees an index's tables and takes nothing, as sa_amd_index_destroy, whose case counts no request; every creating case destroys through it"


# ---------------------------------------------------------------- the driver ----

class Harness:
    def __init__(self, d):
        self.d = d
        self.abi = ra.Abi(sa.library_path())
        self.hooks = ra.Hooks(self.abi)
        self.hip = _hip()
        self.baseline = {}                                            # call -> (kinds, work fields) of the count-only pass

    def ledger_after_release(self):
        self.abi.L.sa_amd_release_cache()
        return self.hooks.ledger()

    def one_call(self, call, c, nth):
        """fresh canaried outputs, the switch at `nth`, the call -> (args, outputs, rc, fired, the requests made, the kinds, the
        runtime's pending error); on the calling thread"""
        c.extra["abi"] = self.abi
        a = call.args(c)
        outs = self.abi.outputs(call.fn, a)
        host_outs = {k: v for k, v in outs.items() if isinstance(v, np.ndarray)}       # (a *_device form's outputs are the case's device buffers)
        ra.fill_canary(host_outs)
        self.hooks.refuse(nth)
        try:
            rc = self.abi.call(call.fn, a)
            fired, kinds = self.hooks.fired(), self.hooks.kinds()
        finally:
            made = self.hooks.refuse(-1)
        peek = int(self.hip.hipPeekAtLastError())
        return a, host_outs, rc, fired, made, kinds, peek

    def stats(self, call):
        return tdb.work_fields({"call": tdb.snapshot(call.getters)}) if call.getters else {}

    def count_pass(self, call):
        """the requests of one successful call, its answers checked, its statistics kept; on a thread of its own"""
        c = call.setup(self.d)
        try:
            def work():
                with tdb.Knobs():
                    a, outs, rc, fired, made, kinds, peek = self.one_call(call, c, 0)
                    assert call.check(c, a, rc), (call.name, "the answers of the count-only pass", rc)
                    assert fired == 0 and peek == 0 and made == len(kinds), (fired, peek, made, kinds)
                    return kinds, self.stats(call)
            return ra.on_a_fresh_thread(work)
        finally:
            self._dispose(c)

    def _dispose(self, c):
        dev = c.extra.get("dev")
        if dev is not None:
            dev.free()
        c.close(self.abi)

    def baseline_of(self, call):
        if call.name not in self.baseline:
            self.baseline[call.name] = self.count_pass(call)
        return self.baseline[call.name]

    def refused(self, call, k):
        kinds, want_stats = self.baseline_of(call)
        assert kinds == call.kinds, (call.name, kinds)
        spilled = []
        before = self.ledger_after_release()
        c = call.setup(self.d)
        try:
            def work():
                with tdb.Knobs():
                    ctx = c
                    a, outs, rc, fired, made, got_kinds, peek = self.one_call(call, ctx, k)
                    where = (call.name, k, call.kinds[k - 1], rc)
                    assert fired == 1 and made >= k and got_kinds[:k] == call.kinds[:k], ("1: the refusal fired once, at request k", where, fired, made)
                    assert rc == ENOMEM or call.check(ctx, a, rc), ("1/3: SA_AMD_ENOMEM, or a success with exact answers", where)
                    key = (call.name, call.kinds[k - 1], k)
                    if rc == ENOMEM:
                        assert key not in FALLBACKS, ("3: a listed fallback answered SA_AMD_ENOMEM", where, FALLBACKS.get(key))
                        allowed = PARTIAL.get(call.name, PARTIAL.get(call.fn[len("sa_amd_"):], (None, "")))[0]
                        written = [name for name, arr in outs.items() if name != allowed and not ra.untouched(arr)]
                        assert not written, ("2: outputs written by a call that answered SA_AMD_ENOMEM", where, written)
                        assert PARTIAL.get(call.fn[len("sa_amd_"):]) is not NULL_HANDLE or int(outs["out"][0]) == 0, ("2: the handle of a failed create", where)
                        assert call.probe is None or call.probe(ctx, self.abi), ("2: the index is not as it was", where)
                    else:
                        assert key in FALLBACKS, ("3: a success that is no listed fallback", where)
                        if FALLBACKS[key] == REDUCED:                  # (asserted behind the ledger: the other properties first)
                            spilled.append(sa.last_host_timing()["workspace_bytes_in_host_memory"])
                    assert peek == 0, ("4: the runtime's error is pending on the thread", where, peek)
                    if rc != ENOMEM and call.redo:                     # the armed call changed the index: the next one starts from a fresh one
                        self._dispose(ctx)
                        ctx = call.setup(self.d)
                    try:
                        a2, _, rc2, _, _, _, peek2 = self.one_call(call, ctx, 0)
                        assert call.check(ctx, a2, rc2) and peek2 == 0, ("5: the un-armed call that follows", where, rc2, peek2)
                        got_stats = self.stats(call)
                        differ = {f: (got_stats.get(f), want_stats[f]) for f in want_stats if got_stats.get(f) != want_stats[f]}
                        assert got_stats.keys() == want_stats.keys() and not differ, ("5: the statistics of the un-armed call", where, differ)
                    finally:
                        if ctx is not c:
                            self._dispose(ctx)
            ra.on_a_fresh_thread(work)
        finally:
            self._dispose(c)
        after = self.ledger_after_release()
        assert after == before, ("6: the ledger (device, pinned) after the case", call.name, k, before, after)
        # 3, the reduced route: the request just refused is never repeated (host_path.hpp, acquire_build_block), so at least the
        # least-used slab of the workspace lives in pinned host memory, however much the device reports as free
        assert all(b > 0 for b in spilled), ("3: the reduced route took no host memory", call.name, k, spilled)


@pytest.fixture(scope="module")
def harness():
    with dirty_blocks.diag_library() as d:
        h = Harness(d)
        d.index(T(), None).close()      # (the pytest thread takes its own read-back block now, outside every case's ledger)
        yield h


@pytest.mark.gpu
def test_a_refusal_is_the_runtimes_own(harness):
    """the first test of the file: a refused request of each seam answers SA_AMD_ENOMEM because the RUNTIME refused the oversized
    request with hipErrorOutOfMemory -- seen through hipPeekAtLastError where the seam's caller has not cleared it yet.  Each seam
    clears the error itself, so the peek behind the call shows hipSuccess; what the runtime answered is read with the same
    oversized request made by the test (SIZE_MAX / 2 bytes, refused on the host: no memory is taken)."""
    hip, abi, hooks = harness.hip, harness.abi, harness.hooks
    huge, p = ctypes.c_size_t((1 << 63) - 1), ctypes.c_void_p()
    hip.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]

    def work():
        answers = {}
        answers["hipMalloc"] = (int(hip.hipMalloc(ctypes.byref(p), huge)), int(hip.hipPeekAtLastError()), int(hip.hipGetLastError()))
        answers["hipHostMalloc"] = (int(hip.hipHostMalloc(ctypes.byref(p), huge, 0x1 | 0x2)), int(hip.hipPeekAtLastError()), int(hip.hipGetLastError()))
        assert int(hip.hipPeekAtLastError()) == 0
        # one seam each: a table (sa_amd_pack's first buffer), a pooled block (sa_amd_bucket_table), a pinned block (the small build)
        for name in ("pack", "bucket_table", "saca_u8-small"):
            call = BY_NAME[name]
            c = call.setup(harness.d)
            a, outs, rc, fired, made, kinds, peek = harness.one_call(call, c, 1)
            answers[name] = (rc, fired, kinds[:1], peek)
        return answers
    answers = ra.on_a_fresh_thread(work)
    print("the runtime's answers to the oversized requests (code, peek, get):", answers)
    assert answers["hipMalloc"] == (2, 2, 2), answers                 # hipErrorOutOfMemory, kept until it is read
    assert answers["hipHostMalloc"] == (2, 2, 2), answers
    assert answers["pack"] == (ENOMEM, 1, ("table",), 0) and answers["bucket_table"] == (ENOMEM, 1, ("device",), 0), answers
    assert answers["saca_u8-small"] == (ENOMEM, 1, ("pinned",), 0), answers


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS, ids=[c.name for c in CALLS])
def test_requests_of_a_call(harness, monkeypatch, call):
    for name, value in call.env.items():
        monkeypatch.setenv(name, value)
    kinds, _ = harness.baseline_of(call)
    assert kinds == call.kinds and len(kinds) <= 64, (call.name, kinds)


REFUSALS = [pytest.param(c, k, id="%s-k%d-%s" % (c.name, k, c.kinds[k - 1])) for c in CALLS for k in range(1, len(c.kinds) + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("call,k", REFUSALS)
def test_refused_request(harness, monkeypatch, call, k):
    for name, value in call.env.items():
        monkeypatch.setenv(name, value)
    harness.refused(call, k)


# ---------------------------------------------------------------- the CPU side ----

def test_every_entry_point_that_takes_memory_has_a_case_or_a_reason():
    """the headers are the whole interface; a call of the table whose entry states no request says so in its case (index_destroy,
    the *_sa copies): the count-only pass asserts it on the GPU"""
    decl = ra.declarations()
    declared = set(decl)
    covered = {c.fn for c in CALLS}
    assert len(declared) >= 134 and covered <= declared and set(NO_CASE) <= declared
    assert not covered & set(NO_CASE), sorted(covered & set(NO_CASE))
    assert declared == covered | set(NO_CASE), sorted(declared ^ (covered | set(NO_CASE)))
    assert all(NO_CASE.values()) and len(BY_NAME) == len(CALLS)
    # the functions the dirty-block table reaches, the eight 32-bit token functions and the Boolean queries are all here
    wanted = {fn for r in tdb.ROUTES for fn in r.fns} | set(tdb.TOK32_FNS) | {"sa_amd_index_doc_match", "sa_amd_index_doc_match_list"}
    assert wanted <= covered | {"sa_amd_saca_batch", "sa_amd_tok_index_destroy", "sa_amd_tok32_index_destroy"}, sorted(wanted - covered)
    assert {"sa_amd_saca_device", "sa_amd_lcp_device", "sa_amd_index_match_stats_device"} <= covered
    assert all(1 <= len(c.kinds) <= 64 or c.name in ("index_destroy", "index_sa", "tok_index_sa", "tok32_index_sa") for c in CALLS)


def test_every_exception_and_fallback_has_its_reason():
    assert all(isinstance(why, str) and len(why) > 20 for why in FALLBACKS.values()) and FALLBACKS
    fns = {c.fn[len("sa_amd_"):] for c in CALLS}
    assert all((name in BY_NAME or name in fns) and out_name and len(sentence) > 20 for name, (out_name, sentence) in PARTIAL.items())
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = " ".join(f.read().split())
    for name, (out_name, sentence) in PARTIAL.items():
        assert " ".join(sentence.split()) in header.replace(" * ", " "), (name, sentence)
    assert len({id_ for id_ in (p.id for p in REFUSALS)}) == len(REFUSALS)


def test_the_outputs_of_every_call_are_read_from_its_declaration():
    """a pointer that is not const is an output: the driver fills it with the canary.  Spot checks of the rule."""
    decl = ra.declarations()
    outs = {fn: [name for _, name, _, output in plist if output] for fn, (_, plist) in decl.items()}
    assert outs["sa_amd_saca_u8"] == ["SA"] and outs["sa_amd_lcp"] == ["LCP"] and outs["sa_amd_index_create"] == ["out"]
    assert outs["sa_amd_index_set_documents"] == [] and outs["sa_amd_index_enable_lcp"] == []
    assert outs["sa_amd_index_doc_tf"] == ["list_off", "docs", "tf", "total_out"]
    assert outs["sa_amd_saca_device"] == ["dSA"] and outs["sa_amd_index_infgram_score"] == ["S", "LO", "HI", "AT_END", "NLO", "NHI"]


def test_the_hook_is_the_diagnostic_librarys_alone():
    """its names stand in csrc/sa_diag.h and in the code under SA_AMD_DIAG, never in the interface headers; the product library
    exports none of them (when it has been built)"""
    names = ("sa_amd_debug_refuse_alloc", "sa_amd_debug_refuse_fired", "sa_amd_debug_refuse_kinds", "sa_amd_debug_live_allocations")
    for text in ts.interface_headers().values():
        assert not any(n in text for n in names)
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "sa_diag.h")) as f:
        diag_h = f.read()
    assert all(n in diag_h for n in names)
    for path in (sa.library_path(),):
        if os.path.exists(path):
            with open(path, "rb") as f:
                blob = f.read()
            assert not any(n.encode() in blob for n in names) and b"refuse_alloc" not in blob


def test_every_call_passes_the_parameters_of_its_declaration():
    """the arguments of every case that needs no device buffer of its own, made with a stand-in for the index: the names are the
    declaration's, in its order, and every output is an array of the case's own (what the driver fills with the canary)"""
    path = os.path.join(os.path.dirname(sa.library_path()), dirty_blocks.DIAG_LIB_NAME)
    abi = ra.Abi(path)                                                # (build() makes it; loading it needs no device)

    class Handle:
        _h = 0
    for call in CALLS:
        if call in DEVICE_CALLS or call.name == "index_destroy":
            continue
        c = Ctx(None)
        c.ix = c.tix = Handle()
        outs = abi.outputs(call.fn, call.args(c))
        ra.fill_canary(outs)
        assert all(ra.untouched(v) for v in outs.values()), call.name
        assert outs or call.fn in ("sa_amd_check_integrity", "sa_amd_index_check_integrity", "sa_amd_index_enable_lcp", "sa_amd_index_set_documents",
                                   "sa_amd_index_enable_doc_freq"), call.name
