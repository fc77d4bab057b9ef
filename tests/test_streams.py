"""Every device entry point on a caller's NON-BLOCKING stream.

The fifteen exported functions that take a `void *stream` promise to work on that stream and to block until done.  On the legacy
null stream, which orders itself against everything, three kinds of mistake cannot be seen: a step (a kernel, a memset of a
control slab, a read-back, a sort pass) queued on another stream than the caller's; a missing or early final wait; and inputs
that are still being produced on the caller's stream when the call is made -- the normal situation under PyTorch.

The shape of every case (`run_case`), with S and R two non-blocking streams of the test's own:
  the input buffers hold a DECOY -- a valid input of the same size --, the real input waits in separate device buffers; the
  outputs hold a canary; a delay chain of CHAIN_K device-to-device copies of 256 MiB is queued on S and, behind it and still on S,
  the copies that put the real input over the decoy and a fill of the work block (a caller's scratch is a recycled buffer whose
  last use may be pending too; the fill value 1 is a legal value of every table a stage keeps there); S must not have drained
  by then; the entry point is called with stream = S and no synchronisation; when it has returned, the outputs are read with
  copies on R alone -- neither S nor the device is waited for -- and compared bit for bit with the CPU reference of the REAL
  input, canaries included; the statistics getters must read what the same call reports on the null stream.
A step that runs early reads the decoy or an unfilled work block and gives a wrong answer; a call that returns early leaves the
canary in the outputs.  The decoy and the fill keep every mis-ordered access in range: a mistake here is a failing test, never
an out-of-range access.  No gate that could keep a stream from draining is used anywhere: the copy chain ends by itself.

The check is one-sided by nature: it proves the presence of an ordering mistake, not its absence.  Two streams may share a
hardware queue, and a step on the wrong stream may still happen to run in the right order.

The expected values come from the references of the features' own suites (imported, not restated), never from the library's
host forms.  The CPU part of the file (not marked gpu) keeps the table of cases complete against the header and checks that
the references of the real and the decoy inputs differ, so that reading the decoy cannot go unnoticed."""
import ctypes
import functools
import inspect
import os
import re
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, Oracle
from test_bwt_abi import bwt_definition
from test_docs_abi import doc_of_definition
from test_lcp_abi import plcp_model
from test_lz77_abi import lpf_definition, parse_definition
from test_match_abi import match_definition
from test_match_abi import spans_definition as match_spans_definition
from test_repeats_abi import keep_first_definition, repeat_lengths_definition
from test_repeats_abi import spans_definition as repeat_spans_definition
from test_score import substituted
from test_score_abi import NAMES as SCORE_NAMES
from test_score_abi import score_definition
from test_substrings import model as substrings_model
from test_substrings_abi import ALL, BY_COVER, node_table

N = 70001                               # above the small-text route (8192) and above 32 769: three levels of minima in LZ and substrings
SEEDS = {"real": 11, "decoy": 12}       # corpus.english_corpus seeds; test_references_of_real_and_decoy_differ keeps them honest
M = 8192                                # query bytes of the index forms
QUERY = {"real": (20000, 5), "decoy": (40000, 6)}     # (where the slice of the real text starts, seed of the 1 % substitutions)
Q_OFF = (0, 3000, 5500, M)              # three documents of the scored query: the host offsets travel on the stream too
DOC_OFF = tuple(sorted({0, N} | {(i * 7919) % N for i in range(1, 300)})) + (N,)      # 300 documents, the last one empty
POS_COUNT = 50000
MIN_LEN = 8                             # of the span queries
SUB_FILTER = (1, 0, 2)
SUB_K = 1000                            # ranked order: below the selected count, so select, cut and sort run
CANARY = 0xA7
HOST_CANARY = -0x5A5A5A5A5A5A5A5B
SCRATCH = 256 << 20                     # bytes of each of the two buffers the delay chain copies between
# Copies of the delay chain.  Measured on the MI355X: 1 copy (the smallest power of two there is) is about 0.1 ms of stream time
# against 0.04-0.1 ms for the whole enqueue, and hipStreamQuery(S) reported hipErrorNotReady behind the enqueue -- input copies
# and work fill included -- in 20 of 20 tries, as it did for 2, 4, 8, 16 and 32.  Chosen: 4 times that (0.44 ms until S has
# drained), because the machine is shared and the host may be descheduled between the enqueue and the call.
CHAIN_K = 4
HIP_NOT_READY = 600                     # hipErrorNotReady
H2D, D2H, D2D = 1, 2, 3
NON_BLOCKING = 1                        # hipStreamNonBlocking
NO_WRAPPER = ("sa_amd_bucket_table_device", "sa_amd_check_integrity_device")    # reached through sa.lib() only
TABLES = ((), ("bkt",), ("lcp",), ("bkt", "lcp"))


# ---------------------------------------------------------------- the references (CPU) ----

@functools.lru_cache(maxsize=None)
def _oracle():
    return Oracle()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def text(which):
    """(text, its suffix array by oracle.sais): computed once, shared, never changed"""
    t = np.ascontiguousarray(corpus.english_corpus(N, SEEDS[which]), dtype=np.uint8)
    return _frozen(t, _oracle().sais(t))


@functools.lru_cache(maxsize=None)
def lcp_of(which):
    t, arr = text(which)
    return _frozen(plcp_model(t, arr)[0])


@functools.lru_cache(maxsize=None)
def lr_of(which):
    t, arr = text(which)
    return _frozen(repeat_lengths_definition(t, arr, lcp_of(which)))


@functools.lru_cache(maxsize=None)
def lpf_of(which):
    return _frozen(*lpf_definition(*text(which)))


@functools.lru_cache(maxsize=None)
def substrings_ref(which):
    t, arr = text(which)
    return (t, arr, lcp_of(which), node_table(lcp_of(which)), {})


@functools.lru_cache(maxsize=None)
def query(which):
    start, seed = QUERY[which]
    return _frozen(np.frombuffer(substituted(text("real")[0].tobytes()[start:start + M], 0.01, seed), dtype=np.uint8).copy())


@functools.lru_cache(maxsize=None)
def positions(which):
    """text positions, some at and behind the end (SA_AMD_MATCH_NONE among them)"""
    rng = np.random.default_rng(SEEDS[which])
    pos = rng.integers(0, N + N // 8, POS_COUNT).astype(np.uint32)
    pos[rng.integers(0, POS_COUNT, 50)] = 0xFFFFFFFF
    return _frozen(pos)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.uint32))


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---------------------------------------------------------------- the table of cases ----

class Variant:
    """one way to call one entry point.
    inputs(which) -> the arrays that go into the input buffers, in order; outs: payload bytes of the device outputs;
    work() -> bytes of the work block; call(env, ins, outs, work, work_bytes, stream) -> what the call gives the host;
    expect(which) -> (the array the call writes at the start of every output -- the rest keeps the canary --, the host value);
    stats() -> the statistics getters of the calling thread; array: the outputs are arrays of one length whatever the input, so
    real and decoy must differ in more than half of the entries"""

    def __init__(self, name, inputs, outs, work, call, expect, stats=None, tables=None, array=True):
        self.name, self.inputs, self.outs, self.work, self.call, self.expect = name, inputs, outs, work, call, expect
        self.stats, self.tables, self.array = stats or (lambda: {}), tables, array


def _both(which):
    return text(which)


def _stats(*getters):
    def read():
        out = {}
        for g in getters:
            out.update({g.__name__ + "." + k: v for k, v in g().items()})
        return out
    return read


def _case_saca():
    def call(env, ins, outs, work, wb, stream):
        sa.saca_device_ptr(ins[0], outs[0], N, work, wb, stream)

    return [Variant("text", lambda w: (text(w)[0],), (4 * (N + 1),), lambda: sa.workspace_bytes(N), call,
                    lambda w: ([text(w)[1]], None), _stats(sa.last_stats))]


def _case_bucket_table():
    def make(with_sa):
        def call(env, ins, outs, work, wb, stream):
            return sa.lib().sa_amd_bucket_table_device(ins[0], ins[1] if with_sa else None, N, outs[0], stream)

        return Variant("from_sa" if with_sa else "from_text", (lambda w: text(w)) if with_sa else (lambda w: (text(w)[0],)),
                       (4 * 65793,), lambda: 0, call, lambda w: ([_oracle().bucket_table(text(w)[0])], 0), array=False)
    return [make(False), make(True)]


def _case_check_integrity():
    """decoy = the real text with the decoy's array (no suffix array of it, but every entry in range), real = a valid pair:
    1 is expected; and the reverse: 0.  Both the streaming work block and the small one."""
    def make(valid, streaming):
        pair = {True: lambda: text("real"), False: lambda: (text("real")[0], text("decoy")[1])}

        def call(env, ins, outs, work, wb, stream):
            return sa.lib().sa_amd_check_integrity_device(ins[0], N, ins[1], work, wb, stream)

        def expect(w):
            t, arr = pair[valid == (w == "real")]()
            return [], int(_oracle().check_integrity(t, arr))

        return Variant(("valid" if valid else "invalid") + ("_streaming" if streaming else "_small"),
                       lambda w: pair[valid == (w == "real")](), (),
                       lambda: sa.lib().sa_amd_check_integrity_work_bytes(N) if streaming else 4 * (N + 1) + 256, call, expect, array=False)
    return [make(v, s) for v in (True, False) for s in (True, False)]


def _case_lcp():
    def call(env, ins, outs, work, wb, stream):
        sa.lcp_device_ptr(ins[0], ins[1], N, outs[0], work, wb, stream)

    return [Variant("array", _both, (4 * (N + 1),), lambda: sa.lcp_work_bytes(N), call, lambda w: ([lcp_of(w)], None),
                    _stats(sa.last_lcp_stats))]


def _case_bwt():
    def call(env, ins, outs, work, wb, stream):
        return sa.bwt_device_ptr(ins[0], ins[1], N, outs[0], work, wb, stream)

    def expect(w):
        b, primary = bwt_definition(*text(w))
        return [b], primary
    return [Variant("transform", _both, (N,), lambda: sa.bwt_work_bytes(N), call, expect)]


def _case_unbwt():
    """the decoy is the transform of the decoy text; `primary` goes by value and is the real one"""
    def call(env, ins, outs, work, wb, stream):
        sa.unbwt_device_ptr(ins[0], N, bwt_definition(*text("real"))[1], outs[0], work, wb, stream)

    return [Variant("inverse", lambda w: (np.ascontiguousarray(bwt_definition(*text(w))[0]),), (N,), lambda: sa.unbwt_work_bytes(N), call,
                    lambda w: ([text(w)[0]], None), _stats(sa.last_unbwt_stats))]


def _case_repeat_lengths():
    def call(env, ins, outs, work, wb, stream):
        sa.repeat_lengths_device_ptr(ins[0], ins[1], N, outs[0], work, wb, stream)

    return [Variant("array", _both, (4 * N,), lambda: sa.repeats_work_bytes(N), call, lambda w: ([_u32(lr_of(w))], None),
                    _stats(sa.last_repeat_stats, sa.last_lcp_stats))]


def _spans_of(which, mode):
    if mode == sa.REPEATS_ALL:
        return repeat_spans_definition(lr_of(which), MIN_LEN)[0]
    t, arr = text(which)
    return keep_first_definition(t, arr, lcp_of(which), MIN_LEN)[0]


def _case_repeat_spans():
    def make(mode, above):
        def capacity():
            total = _spans_of("real", mode).shape[0]
            return total + 5 if above else total // 2

        def call(env, ins, outs, work, wb, stream):
            if above:                                                 # through the wrapper; below: the host word holds a canary
                return sa.repeat_spans_device_ptr(ins[0], ins[1], N, MIN_LEN, mode, outs[0], capacity(), work, wb, stream)
            cnt = ctypes.c_int64(HOST_CANARY)
            assert sa.lib().sa_amd_repeat_spans_device(ins[0], ins[1], N, MIN_LEN, mode, outs[0], capacity(), ctypes.byref(cnt), work, wb, stream) == 0
            return int(cnt.value)

        def expect(w):
            sp = _spans_of(w, mode)
            return [_u32(sp[:capacity()])], int(sp.shape[0])
        return Variant(("all" if mode == sa.REPEATS_ALL else "keep_first") + ("_fits" if above else "_cut"), _both,
                       (lambda: (8 * capacity(),)), lambda: sa.repeats_work_bytes(N), call, expect, _stats(sa.last_repeat_stats, sa.last_lcp_stats),
                       array=False)
    return [make(m, a) for m in (sa.REPEATS_ALL, sa.REPEATS_KEEP_FIRST) for a in (True, False)]


def _case_lpf():
    def call(env, ins, outs, work, wb, stream):
        sa.lpf_device_ptr(ins[0], ins[1], N, outs[0], outs[1], work, wb, stream)

    return [Variant("arrays", _both, (4 * N, 4 * N), lambda: sa.lz_work_bytes(N), call,
                    lambda w: ([_u32(lpf_of(w)[0]), _u32(lpf_of(w)[1])], None), _stats(sa.last_lz_stats, sa.last_lcp_stats))]


def _case_lz77():
    def make(above):
        def capacity():
            total = parse_definition(*lpf_of("real")).shape[0]
            return total + 5 if above else total // 2

        def call(env, ins, outs, work, wb, stream):
            if above:
                return sa.lz77_device_ptr(ins[0], ins[1], N, outs[0], capacity(), work, wb, stream)
            cnt = ctypes.c_int64(HOST_CANARY)
            assert sa.lib().sa_amd_lz77_device(ins[0], ins[1], N, outs[0], capacity(), ctypes.byref(cnt), work, wb, stream) == 0
            return int(cnt.value)

        def expect(w):
            ph = parse_definition(*lpf_of(w))
            return [_u32(ph[:capacity()])], int(ph.shape[0])
        return Variant("fits" if above else "cut", _both, (lambda: (8 * capacity(),)), lambda: sa.lz_work_bytes(N), call, expect,
                       _stats(sa.last_lz_stats, sa.last_lcp_stats), array=False)
    return [make(True), make(False)]


def _case_substrings():
    def make(order, above):
        k = 0 if order == ALL else SUB_K

        def capacity():
            total = substrings_model(substrings_ref("real"), SUB_FILTER, order, k)[0].shape[0]
            return total + 5 if above else total // 2

        def call(env, ins, outs, work, wb, stream):
            q = sa.SubstrQuery(SUB_FILTER[0], SUB_FILTER[1], SUB_FILTER[2], order, k)
            if above:
                return sa.substrings_device_ptr(ins[0], ins[1], N, q, outs[0], outs[1], capacity(), work, wb, stream)
            total = ctypes.c_int64(HOST_CANARY)
            assert sa.lib().sa_amd_substrings_device(ins[0], ins[1], N, ctypes.byref(q), outs[0], outs[1], capacity(), ctypes.byref(total), work, wb,
                                                     stream) == 0
            return int(total.value)

        def expect(w):
            rows, pos, _ = substrings_model(substrings_ref(w), SUB_FILTER, order, k)
            return [_u32(rows[:capacity()]), _u32(pos[:capacity()])], int(rows.shape[0])
        return Variant(("all" if order == ALL else "by_cover") + ("_fits" if above else "_cut"), _both, (lambda: (16 * capacity(), 4 * capacity())),
                       lambda: sa.substrings_work_bytes(N), call, expect, _stats(sa.last_substr_stats, sa.last_lcp_stats), array=False)
    return [make(o, a) for o in (ALL, BY_COVER) for a in (True, False)]


def _tables_name(tables):
    return "+".join(tables) if tables else "plain"


@functools.lru_cache(maxsize=None)
def _match(which):
    return _frozen(*match_definition(*text("real"), query(which), 1 << 20))


def _case_match_stats():
    def make(tables):
        def call(env, ins, outs, work, wb, stream):
            sa.match_stats_device_ptr(env.index(tables), ins[0], M, 1 << 20, outs[0], outs[1], work, wb, stream)

        def expect(w):
            ml, pos = _match(w)
            return [_u32(ml), _u32(pos)], None
        return Variant(_tables_name(tables), lambda w: (query(w),), (4 * M, 4 * M), lambda: sa.match_work_bytes(M), call, expect,
                       _stats(sa.last_match_stats), tables=tables)
    return [make(t) for t in TABLES]


@functools.lru_cache(maxsize=None)
def _match_spans(which):
    return match_spans_definition(*text("real"), query(which), MIN_LEN)[0]


def _case_match_spans():
    def make(tables, above):
        def capacity():
            total = _match_spans("real").shape[0]
            return total + 5 if above else total // 2

        def call(env, ins, outs, work, wb, stream):
            if above:
                return sa.match_spans_device_ptr(env.index(tables), ins[0], M, MIN_LEN, outs[0], capacity(), work, wb, stream)
            cnt = ctypes.c_int64(HOST_CANARY)
            assert sa.lib().sa_amd_index_match_spans_device(env.index(tables)._h, ins[0], M, MIN_LEN, outs[0], capacity(), ctypes.byref(cnt), work,
                                                            wb, stream) == 0
            return int(cnt.value)

        def expect(w):
            sp = _match_spans(w)
            return [_u32(sp[:capacity()])], int(sp.shape[0])
        return Variant(_tables_name(tables) + ("_fits" if above else "_cut"), lambda w: (query(w),), (lambda: (8 * capacity(),)),
                       lambda: sa.match_work_bytes(M), call, expect, _stats(sa.last_match_stats), tables=tables, array=False)
    return [make(t, a) for t in TABLES for a in (True, False)]


def _case_doc_of():
    def call(env, ins, outs, work, wb, stream):
        sa.doc_of_device_ptr(env.index(()), ins[0], POS_COUNT, outs[0], stream)

    return [Variant("positions", lambda w: (positions(w),), (4 * POS_COUNT,), lambda: 0, call,
                    lambda w: ([_u32(doc_of_definition(DOC_OFF, N, positions(w)))], None), tables=())]


@functools.lru_cache(maxsize=None)
def _score(which):
    d = score_definition(text("real")[0].tobytes(), text("real")[1], query(which).tobytes(), np.array(Q_OFF), 1, sa.SCORE_MAX_CONTEXT)
    return {k: _frozen(v) for k, v in d.items()}


def _case_score():
    """every table combination, the default group cap and 0: at 0 the long pass and its second read-back run"""
    def make(tables, cap):
        def call(env, ins, outs, work, wb, stream):
            prev = sa.score_set_group_cap(cap)
            try:
                sa.infgram_score_device_ptr(env.index(tables), ins[0], M, 1, sa.SCORE_MAX_CONTEXT, *outs, work, wb, doc_offsets=list(Q_OFF),
                                            stream=stream)
            finally:
                sa.score_set_group_cap(prev)

        def expect(w):
            d = _score(w)
            return [d[k].astype(np.uint8 if k == "at_end" else np.uint32) for k in SCORE_NAMES], None
        return Variant(_tables_name(tables) + ("_cap0" if cap == 0 else ""), lambda w: (query(w),), tuple(M if k == "at_end" else 4 * M for k in SCORE_NAMES),
                       lambda: sa.score_work_bytes(M, len(Q_OFF) - 1), call, expect, _stats(sa.last_score_stats), tables=tables, array=False)
    return [make(t, c) for t in TABLES for c in (-1, 0)]


CASES = {
    "sa_amd_saca_device": _case_saca(),
    "sa_amd_bucket_table_device": _case_bucket_table(),
    "sa_amd_check_integrity_device": _case_check_integrity(),
    "sa_amd_lcp_device": _case_lcp(),
    "sa_amd_bwt_device": _case_bwt(),
    "sa_amd_unbwt_device": _case_unbwt(),
    "sa_amd_repeat_lengths_device": _case_repeat_lengths(),
    "sa_amd_repeat_spans_device": _case_repeat_spans(),
    "sa_amd_lpf_device": _case_lpf(),
    "sa_amd_lz77_device": _case_lz77(),
    "sa_amd_substrings_device": _case_substrings(),
    "sa_amd_index_match_stats_device": _case_match_stats(),
    "sa_amd_index_match_spans_device": _case_match_spans(),
    "sa_amd_index_doc_of_device": _case_doc_of(),
    "sa_amd_index_infgram_score_device": _case_score(),
}
EVERY = [pytest.param(fn, v, id=fn[len("sa_amd_"):] + "-" + v.name) for fn, variants in CASES.items() for v in variants]


def _outs(v):
    return tuple(v.outs() if callable(v.outs) else v.outs)


# ---------------------------------------------------------------- the guard and the decoys (CPU) ----

def interface_headers():
    """name -> text without its comments of include/suffix_array_amd.h and of every suffix_array_amd_*.h it includes: the whole
    interface.  A sub-header is seen because the main header names it, not because this function does."""
    def plain(name):
        with open(os.path.join(ROOT, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    main = "suffix_array_amd.h"
    out = {main: plain(main)}
    for name in re.findall(r'^#include "(suffix_array_amd_\w+\.h)"$', out[main], re.M):
        out[name] = plain(name)
    on_disk = {f for f in os.listdir(os.path.join(ROOT, "include")) if re.fullmatch(r"suffix_array_amd(_\w+)?\.h", f)}
    assert set(out) == on_disk, sorted(on_disk ^ set(out))            # no C header lies beside them that the main one does not bring in
    return out


def declarations_with_a_stream():
    """name -> parameter list of every declaration of the interface (interface_headers) that takes `void *stream`"""
    header = "\n".join(interface_headers().values())
    found = {}
    for name, params in re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", header):
        params = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
        if "void *stream" in params:
            found[name] = params
    return found


def wrapper_name(fn):
    base = fn[len("sa_amd_"):]
    return (base[len("index_"):] if base.startswith("index_") else base) + "_ptr"


def test_the_table_has_a_case_for_every_entry_point_with_a_stream():
    decl = declarations_with_a_stream()
    assert len(decl) >= 15 and set(decl) == set(CASES)
    # the scan follows the main header's includes; the sub-headers declare host-pointer forms only, so the count is the main header's
    headers = interface_headers()
    assert len(headers) >= 3 and len(decl) == 15
    assert all("void *stream" not in text for name, text in headers.items() if name != "suffix_array_amd.h")
    assert all(variants for variants in CASES.values())


def test_every_entry_point_has_a_wrapper_whose_stream_defaults_to_the_null_stream():
    """... or is listed in NO_WRAPPER.  `stream` is the wrapper's last parameter; only `stats` may follow it, as it does in C"""
    for fn, params in declarations_with_a_stream().items():
        name = wrapper_name(fn)
        if fn in NO_WRAPPER:
            assert not hasattr(sa, name), fn
            continue
        assert name in sa.__all__ and callable(getattr(sa, name)), fn
        sig = inspect.signature(getattr(sa, name)).parameters
        names = list(sig)
        assert "stream" in names and sig["stream"].default == 0, fn
        assert names[names.index("stream") + 1:] in ([], ["stats"]), fn
        # a handle is a pointer: it crosses ctypes as one, whole
        assert getattr(sa.lib(), fn).argtypes[params.index("void *stream")] is ctypes.c_void_p, fn
    for fn in NO_WRAPPER:
        assert getattr(sa.lib(), fn).argtypes[declarations_with_a_stream()[fn].index("void *stream")] is ctypes.c_void_p, fn


@pytest.mark.parametrize("fn,v", EVERY)
def test_references_of_real_and_decoy_differ(fn, v):
    """a step that reads the decoy must give another answer: the inputs have the same sizes, the references differ -- arrays of
    a fixed length in more than half of their entries"""
    real, decoy = v.inputs("real"), v.inputs("decoy")
    assert [(a.dtype, a.shape) for a in real] == [(a.dtype, a.shape) for a in decoy]
    assert any(not np.array_equal(a, b) for a, b in zip(real, decoy))
    (outs_r, host_r), (outs_d, host_d) = v.expect("real"), v.expect("decoy")
    assert len(outs_r) == len(_outs(v)) and all(a.nbytes <= size for a, size in zip(outs_r, _outs(v)))
    if not outs_r:
        assert host_r != host_d
    for a, b in zip(outs_r, outs_d):
        assert a.dtype == b.dtype and a.dtype in (np.uint8, np.uint32)
        assert a.shape != b.shape or not np.array_equal(a, b), (fn, v.name)
        if v.array:
            assert a.shape == b.shape and a.ndim == 1
            differ = int(np.count_nonzero(a != b))
            assert 2 * differ > a.size, (fn, v.name, differ, a.size)


# ---------------------------------------------------------------- the device side ----

def _hip():
    hip = ctypes.CDLL("libamdhip64.so")                               # (already in the process: the product library links it)
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemset.argtypes = [vp, ctypes.c_int, ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(vp), ctypes.c_uint]
    for fn in ("hipStreamDestroy", "hipStreamQuery", "hipStreamSynchronize"):
        getattr(hip, fn).argtypes = [vp]
    return hip


class Env:
    """what the module shares: the HIP entry points, the two scratch buffers of the delay chain, one index per table combination
    (created in the ordinary way from the real text; the plain one holds the document collection)"""

    def __init__(self):
        sa.lib()
        self.hip = _hip()
        self.scratch = [self.malloc(SCRATCH), self.malloc(SCRATCH)]
        self._index = {}
        self._null = {}
        self._lock = threading.Lock()

    def malloc(self, size):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(int(size), 1)) == 0
        return p.value

    def stream(self):
        s = ctypes.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(ctypes.byref(s), NON_BLOCKING) == 0 and s.value
        return s.value

    def reader(self):
        """a stream that has made one device -> host copy already: what a stream's first copy costs (its queue, the staging
        buffers) would otherwise give a call that returned early the time to finish behind the test's back"""
        s = self.stream()
        word = np.zeros(64, dtype=np.uint8)
        assert self.hip.hipMemcpyAsync(word.ctypes.data, self.scratch[0], word.size, D2H, s) == 0
        assert self.hip.hipStreamSynchronize(s) == 0
        return s

    def index(self, tables):
        with self._lock:
            if tables not in self._index:
                ix = sa.DeviceIndex(*text("real"))
                if "bkt" in tables:
                    ix.buckets()
                if "lcp" in tables:
                    ix.enable_lcp()
                if not tables:
                    ix.set_documents(np.array(DOC_OFF, dtype=np.uint32))
                self._index[tables] = ix
            return self._index[tables]

    def queue_chain(self, stream, copies=None):
        a, b = self.scratch
        for i in range(CHAIN_K if copies is None else copies):
            assert self.hip.hipMemcpyAsync(b if i % 2 == 0 else a, a if i % 2 == 0 else b, SCRATCH, D2D, stream) == 0

    def close(self):
        for ix in self._index.values():
            ix.close()
        for p in self.scratch:
            self.hip.hipFree(p)


@pytest.fixture(scope="module")
def env():
    e = Env()
    try:
        yield e
    finally:
        e.close()


class Buffers:
    """the device buffers of one call: inputs, the sources the real input waits in, outputs with 256 canary bytes on either side,
    the work block and the source of its fill.  fill(bytes) -> the array the source of the fill holds (default: the word 1)"""

    def __init__(self, env, v, fill=None):
        self.env, self.hip, self.v = env, env.hip, v
        self.fill_source = fill if fill is not None else (lambda size: np.ones(size // 4, dtype=np.uint32))
        self.all = []
        self.sizes = [a.nbytes for a in v.inputs("real")]
        self.ins = [self.take(s + 16) for s in self.sizes]
        self.srcs = [self.take(s + 16) for s in self.sizes]
        self.out_sizes = _outs(v)
        self.outs = [self.take(s + 512) for s in self.out_sizes]
        self.wb = int(v.work())
        self.work = self.take(self.wb)
        self.fill = self.take(self.wb)

    def take(self, size):
        p = self.env.malloc(size)
        self.all.append(p)
        return p

    def upload(self, dst, arr):
        a = np.ascontiguousarray(arr)
        if a.nbytes:
            assert self.hip.hipMemcpy(dst, a.ctypes.data, a.nbytes, H2D) == 0

    def load(self, ins_from, srcs_from=None):
        """synchronously: `ins_from` into the inputs, `srcs_from` into the sources, the canary into the outputs, the fill into
        its source (ones by default); then the device is idle"""
        for p, a in zip(self.ins, self.v.inputs(ins_from)):
            self.upload(p, a)
        if srcs_from:
            for p, a in zip(self.srcs, self.v.inputs(srcs_from)):
                self.upload(p, a)
        for p, s in zip(self.outs, self.out_sizes):
            assert self.hip.hipMemset(p, CANARY, s + 512) == 0
        if self.wb:
            self.upload(self.fill, self.fill_source(self.wb))
        assert self.hip.hipDeviceSynchronize() == 0

    def queue_real_input(self, stream):
        for p, q, s in zip(self.ins, self.srcs, self.sizes):
            assert self.hip.hipMemcpyAsync(p, q, s, D2D, stream) == 0
        if self.wb:
            assert self.hip.hipMemcpyAsync(self.work, self.fill, self.wb, D2D, stream) == 0

    def call(self, stream):
        return self.v.call(self.env, self.ins, [p + 256 for p in self.outs], self.work, self.wb, stream)

    def read(self, stream):
        """the outputs, canaries included, by copies on `stream` and a wait for that stream alone"""
        raw = [np.zeros(s + 512, dtype=np.uint8) for s in self.out_sizes]
        for p, r in zip(self.outs, raw):
            assert self.hip.hipMemcpyAsync(r.ctypes.data, p, r.size, D2H, stream) == 0
        assert self.hip.hipStreamSynchronize(stream) == 0
        return raw

    def free(self):
        for p in self.all:
            self.hip.hipFree(p)


def compare(v, raw, host, which="real", where=""):
    outs, want = v.expect(which)
    assert host == want, (where, v.name, host, want)
    for k, (r, e) in enumerate(zip(raw, outs)):
        e = _bytes(e)
        assert np.all(r[:256] == CANARY) and np.all(r[256 + e.size:] == CANARY), (where, v.name, k, "canary")
        bad = np.flatnonzero(r[256:256 + e.size] != e)
        assert bad.size == 0, (where, v.name, k, bad.size, bad[:4].tolist(), r[256:256 + e.size][bad[:4]].tolist(), e[bad[:4]].tolist())


def null_stream_stats(env, v):
    """the statistics the same call reports on the null stream for the real input (its outputs checked as well); once per variant"""
    with env._lock:
        known = env._null.get(id(v))
    if known is None:
        b = Buffers(env, v)
        try:
            b.load("real")
            host = b.call(0)
            known = v.stats()
            raw = [np.zeros(s + 512, dtype=np.uint8) for s in b.out_sizes]
            for p, r in zip(b.outs, raw):
                assert env.hip.hipMemcpy(r.ctypes.data, p, r.size, D2H) == 0
            compare(v, raw, host, where="null stream")
        finally:
            b.free()
        with env._lock:
            env._null[id(v)] = known
    return known


def run_case(env, v, barrier=None):
    """the case shape of the module docstring"""
    want_stats = null_stream_stats(env, v)
    hip = env.hip
    S, R = env.stream(), env.reader()
    b = Buffers(env, v)
    try:
        b.load("decoy", "real")
        if barrier is not None:
            barrier.wait(60)
        env.queue_chain(S)
        b.queue_real_input(S)
        state = hip.hipStreamQuery(S)
        assert state == HIP_NOT_READY, f"hipStreamQuery(S) = {state}: the delay chain of {CHAIN_K} copies is too short, S has drained before the call"
        host = b.call(S)
        stats = v.stats()
        raw = b.read(R)
        compare(v, raw, host, where="stream")
        assert stats == want_stats, (v.name, stats, want_stats)
    finally:
        hip.hipStreamSynchronize(S)
        b.free()
        hip.hipStreamDestroy(S)
        hip.hipStreamDestroy(R)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,v", EVERY)
def test_entry_point_on_a_busy_non_blocking_stream(env, fn, v):
    run_case(env, v)


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [("sa_amd_lcp_device", "sa_amd_lz77_device"),
                                          ("sa_amd_index_match_stats_device", "sa_amd_index_infgram_score_device"),
                                          ("sa_amd_saca_device", "sa_amd_substrings_device")])
def test_two_threads_at_once(env, first, second):
    """each thread has its own stream, buffers and work block (the index is shared): its outputs and its thread-local statistics
    are its own"""
    pair = [CASES[first][0], CASES[second][-1]]
    for v in pair:
        null_stream_stats(env, v)                                     # (the baselines first, one after the other)
    barrier = threading.Barrier(2)
    errors = []

    def work(v):
        try:
            run_case(env, v, barrier)
        except BaseException as e:                                    # noqa: B902 -- handed to the main thread
            barrier.abort()
            errors.append((v.name, e))
    threads = [threading.Thread(target=work, args=(v,)) for v in pair]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0][1]


def _twice(env, stages, inputs, check):
    """two entry points back to back on S, the second reading what the first left on the device: a delay chain in front of the
    first only and no synchronisation between the calls beyond what the calls do themselves.  stages(S, ins, mid, out, works)
    makes both calls; `mid` and `out` are canaried buffers"""
    hip = env.hip
    S, R = env.stream(), env.reader()
    taken = []

    def take(size):
        taken.append(env.malloc(size))
        return taken[-1]
    try:
        real, decoy = inputs("real"), inputs("decoy")
        ins, srcs = [take(a.nbytes + 16) for a in real], [take(a.nbytes + 16) for a in real]
        for p, q, a, d in zip(ins, srcs, real, decoy):
            assert hip.hipMemcpy(p, np.ascontiguousarray(d).ctypes.data, d.nbytes, H2D) == 0
            assert hip.hipMemcpy(q, np.ascontiguousarray(a).ctypes.data, a.nbytes, H2D) == 0
        size = 4 * (N + 1) + 512
        mid, out = take(size), take(size)
        for p in (mid, out):
            assert hip.hipMemset(p, CANARY, size) == 0
        works = [(take(wb), wb) for wb in check["work"]]
        assert hip.hipDeviceSynchronize() == 0
        env.queue_chain(S)
        for p, q, a in zip(ins, srcs, real):
            assert hip.hipMemcpyAsync(p, q, a.nbytes, D2D, S) == 0
        assert hip.hipStreamQuery(S) == HIP_NOT_READY, f"the delay chain of {CHAIN_K} copies is too short"
        host = stages(S, ins, mid + 256, out + 256, works)
        raw = [np.zeros(size, dtype=np.uint8) for _ in range(2)]
        for p, r in zip((mid, out), raw):
            assert hip.hipMemcpyAsync(r.ctypes.data, p, size, D2H, R) == 0
        assert hip.hipStreamSynchronize(R) == 0
        for r, e, name in zip(raw, check["expect"], ("first", "second")):
            assert np.all(r[:256] == CANARY) and np.all(r[256 + e.size:] == CANARY), name
            assert np.array_equal(r[256:256 + e.size], e), name
        return host
    finally:
        hip.hipStreamSynchronize(S)
        for p in taken:
            hip.hipFree(p)
        hip.hipStreamDestroy(S)
        hip.hipStreamDestroy(R)


@pytest.mark.gpu
def test_the_same_stream_twice_saca_then_lcp(env):
    def stages(S, ins, mid, out, works):
        sa.saca_device_ptr(ins[0], mid, N, works[0][0], works[0][1], S)
        sa.lcp_device_ptr(ins[0], mid, N, out, works[1][0], works[1][1], S)

    _twice(env, stages, lambda w: (text(w)[0],),
           {"work": (sa.workspace_bytes(N), sa.lcp_work_bytes(N)), "expect": (_bytes(text("real")[1]), _bytes(lcp_of("real")))})


@pytest.mark.gpu
def test_the_same_stream_twice_bwt_then_unbwt(env):
    b, primary = bwt_definition(*text("real"))

    def stages(S, ins, mid, out, works):
        got = sa.bwt_device_ptr(ins[0], ins[1], N, mid, works[0][0], works[0][1], S)
        sa.unbwt_device_ptr(mid, N, got, out, works[1][0], works[1][1], S)
        return got

    got = _twice(env, stages, text, {"work": (sa.bwt_work_bytes(N), sa.unbwt_work_bytes(N)), "expect": (_bytes(b), _bytes(text("real")[0]))})
    assert got == primary
