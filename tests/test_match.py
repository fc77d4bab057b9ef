"""GPU suite for matching a query against the device index: every route (host pointers, device pointers with misaligned queries
and canaries, DeviceIndex, SuffixArray) against the numpy definitions of test_match_abi.py over the oracle's suffix array; the
pin to sa_amd_index_search on the explicit windows; invariance under the bucket and LCP tables; the group-cap routes; every
group width; the work bound; spans, capacity, errors; a text of a million bytes against the oracle library's matching
statistics; the top of the size range, threads."""
import ctypes
import hashlib
import json
import math
import os
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, adversarial_cases, fibonacci_word
from test_lcp import _Dev
from test_match_abi import (CAPS, NONE, STAGE_MAX, _u8, long_positions_definition, match_definition, oracle_match_stats, queries,
                            spans_definition, stats_definition, union_spans)

pytestmark = pytest.mark.gpu

TILE = sa.MATCH_TILE
CANARY = 0xA5
N_ABOVE = (1 << 30) + 4097
_CASES = adversarial_cases()
_WANTS = ((True, True), (True, False), (False, True))


_MEMO = {}
LANES = (4, 8, 16)
_ACROSS_WIDTHS = {}


def same_for_every_width(key, lanes, *arrays):
    """what the first group width answered for `key` is what every other width answers, bit for bit (by digest)"""
    got = tuple(hashlib.sha256(np.asarray(a).astype(np.uint32).tobytes()).digest() for a in arrays)
    first = _ACROSS_WIDTHS.setdefault(key, (lanes, got))
    assert first[1] == got, (key, "lanes", first[0], lanes)


def _memo(fn, t, arr, q, cap):
    key = (fn.__name__, t.size, hash(t.tobytes()), q.size, hash(q.tobytes()), cap)
    if key not in _MEMO:
        _MEMO[key] = fn(t, arr, q, cap)
    return _MEMO[key]


def match_model(t, arr, q, cap):
    """the numpy definitions, computed once per (text, query, cap) and left unchanged"""
    return _memo(match_definition, t, arr, q, cap)


def spans_model(t, arr, q, k):
    return _memo(spans_definition, t, arr, q, k)


def _golden():
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "manifest.json")) as f:
        names = sorted(json.load(f))
    return {name: (np.fromfile(os.path.join(gold, name + ".text"), dtype=np.uint8),
                   np.fromfile(os.path.join(gold, name + ".sa.u32le"), dtype="<u4")) for name in names}


def bytes_bound(n, m, cap, st, long_mask):
    """the work bound of DESIGN.md section 15, summed over the positions: the group path for every position, the wave path on
    top for those that left it"""
    c = np.minimum(cap, m - np.arange(m)).astype(np.int64)
    steps = math.ceil(math.log2(n + 1)) + 3 if n else 3
    total = int(np.sum(steps * (np.minimum(c, st["group_cap"]) + 4 * st["group_lanes"])))
    cl = c[long_mask]
    if st["route_long"]:
        log_p = 1
        while (1 << log_p) < n + 2:
            log_p += 1
        total += int(np.sum(2 * cl + 128 * log_p))
    else:
        total += int(np.sum(steps * (cl + 64)))
    return total


def check_stats(ml, m, n, cap, group_cap=64, st=None, spans=None, lanes=None):
    st = sa.last_match_stats() if st is None else st
    for key, val in stats_definition(ml).items():
        assert st[key] == val, (key, st)
    ge = min(group_cap, STAGE_MAX)
    assert st["group_cap"] == ge and st["tile"] == TILE and st["group_lanes"] in (4, 8, 16)
    if lanes is not None:
        assert st["group_lanes"] == lanes, st
    assert st["long_positions"] == long_positions_definition(ml, m, cap, group_cap), st
    c = np.minimum(cap, m - np.arange(m))
    assert st["compared_bytes"] <= bytes_bound(n, m, cap, st, (c > ge) & (ml >= ge)), st
    if m:
        assert 1 <= st["readbacks"] <= 2
    if spans is None:
        assert st["spans"] == 0 and st["covered_bytes"] == 0 and st["flagged"] == 0
    else:
        sp, flagged = spans
        assert st["spans"] == sp.shape[0] and st["flagged"] == flagged.size
        assert st["covered_bytes"] == int(np.sum(sp[:, 1] - sp[:, 0])) if sp.size else st["covered_bytes"] == 0
    return st


def stats_on_device(ix, q, cap, offset=0, want=(True, True)):
    """sa_amd_index_match_stats_device on hipMalloc'ed buffers: `offset` bytes of misalignment in front of the query, 256 canary
    bytes on either side of both outputs"""
    m = q.size
    wb = sa.match_work_bytes(m)
    with _Dev(m + 16, 4 * m + 512, 4 * m + 512, wb) as d:
        dQ, dM, dP, dW = d.p
        for p in (dM, dP):
            assert d.hip.hipMemset(p, CANARY, 4 * m + 512) == 0
        if m:
            assert d.hip.hipMemcpy(dQ + offset, q.ctypes.data, m, 1) == 0
        sa.match_stats_device_ptr(ix, dQ + offset, m, cap, dM + 256 if want[0] else 0, dP + 256 if want[1] else 0, dW, wb)
        out = []
        for p, on in ((dM, want[0]), (dP, want[1])):
            raw = np.zeros(4 * m + 512, dtype=np.uint8)
            assert d.hip.hipMemcpy(raw.ctypes.data, p, raw.size, 2) == 0
            assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 4 * m:] == CANARY)
            if not on:
                assert np.all(raw == CANARY)
            out.append(raw[256:256 + 4 * m].view(np.uint32).astype(np.int64))
    return out


def spans_on_device(ix, q, k, capacity, offset=0):
    m = q.size
    wb = sa.match_work_bytes(m)
    with _Dev(m + 16, 8 * capacity + 512, wb) as d:
        dQ, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * capacity + 512) == 0
        if m:
            assert d.hip.hipMemcpy(dQ + offset, q.ctypes.data, m, 1) == 0
        count = sa.match_spans_device_ptr(ix, dQ + offset, m, k, dO + 256, capacity, dW, wb)
        raw = np.zeros(8 * capacity + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
    assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 8 * capacity:] == CANARY)
    wrote = min(count, capacity)
    assert np.all(raw[256 + 8 * wrote:256 + 8 * capacity] == CANARY)
    return count, raw[256:256 + 8 * wrote].view(np.uint32).reshape(-1, 2).astype(np.int64)


def host_call(ix, q, cap, want=(True, True)):
    m = q.size
    bufs = [np.full(m + 128, 0xA5A5A5A5, dtype=np.uint32) for _ in range(2)]
    args = [b[64:].ctypes.data if on else None for b, on in zip(bufs, want)]
    assert sa.lib().sa_amd_index_match_stats(ix._h, q.ctypes.data if m else None, m, cap, args[0], args[1]) == 0
    for b, on in zip(bufs, want):
        assert np.all(b[:64] == 0xA5A5A5A5) and np.all(b[64 + m:] == 0xA5A5A5A5)
        if not on:
            assert np.all(b == 0xA5A5A5A5)
    return [b[64:64 + m].astype(np.int64) for b in bufs]


def pin_to_search(pin_ix, q, cap, ml, pos):
    """what the parent's only route reports for the explicit windows, on an index without a bucket table"""
    qb = q.tobytes()
    r = pin_ix.search([qb[j:j + cap] for j in range(len(qb))])
    on = r["lcp_len"] > 0
    assert np.array_equal(on, ml > 0)
    assert np.array_equal(r["lcp_len"][on], ml[on]) and np.array_equal(r["lcp_start"][on], pos[on])


def check_text(name, t, arr, caps=CAPS, seed=0):
    """every query kind and cap on one text: host call with both outputs against the model and the parent's route, the device call
    with a rotating misalignment and choice of outputs"""
    n = t.size
    ix = sa.DeviceIndex(t, arr)
    turn = 0
    for qname, q in queries(t, seed).items():
        m = q.size
        for cap in tuple(caps) + (m + 5,):
            ml, pos = match_model(t, arr, q, cap)
            got = host_call(ix, q, cap)
            assert np.array_equal(got[0], ml) and np.array_equal(got[1], pos), (name, qname, cap)
            check_stats(ml, m, n, cap)
            if qname == "absent":
                assert not ml.any() and np.all(pos == NONE)
            if m * cap <= 1 << 22 and m:
                pin_to_search(ix, q, cap, ml, pos)
            want = _WANTS[turn % 3]
            dev = stats_on_device(ix, q, cap, turn % 8, want)
            assert (not want[0] or np.array_equal(dev[0], ml)) and (not want[1] or np.array_equal(dev[1], pos)), (name, qname, cap, turn)
            turn += 1
    ix.close()


@pytest.mark.parametrize("name", sorted(_CASES))
def test_adversarial_cases(oracle, name):
    t = _u8(_CASES[name])
    check_text(name, t, oracle.sais(t))


def test_golden_fixtures():
    for name, (t, arr) in _golden().items():
        check_text(name, t, arr)


@pytest.mark.parametrize("b", [b"", b"a", b"ab", b"aa"])
def test_tiny_texts(oracle, b):
    t = _u8(b)
    check_text(b, t, oracle.sais(t))


def test_known_answers():
    ix = sa.DeviceIndex(b"banana")
    ml, pos = ix.match_stats(b"bandana", 8)
    assert ml.dtype == np.uint32 and pos.dtype == np.uint32
    assert ml.tolist() == [3, 2, 1, 0, 3, 2, 1] and pos.tolist() == [0, 1, 2, NONE, 3, 4, 5]
    st = sa.last_match_stats()
    assert (st["positions"], st["matched"], st["longest"], st["longest_pos"], st["ml_sum"]) == (7, 6, 3, 0, 12)
    assert ix.match_spans(b"bandana", 2).tolist() == [[0, 3], [4, 7]] and ix.match_spans(b"bandana", 4).shape == (0, 2)
    ml, pos = ix.match_stats(b"", 3)
    assert ml.shape == (0,) and pos.shape == (0,) and sa.last_match_stats()["longest_pos"] == -1
    assert ix.match_spans(b"", 3).shape == (0, 2)
    s = sa.SuffixArray(b"banana")
    assert s.match_stats(b"bandana", 8)[1].tolist() == [0, 1, 2, NONE, 3, 4, 5] and s.match_spans(b"bandana", 3).tolist() == [[0, 3], [4, 7]]
    ix.close()


@pytest.mark.parametrize("lanes", LANES)
def test_every_offset_and_output_choice(oracle, lanes):
    t = corpus.english_corpus(3000, 4)
    arr = oracle.sais(t)
    q = queries(t, 2)["changed"][:2 * TILE + 77]
    prev = sa.match_set_group_lanes(lanes)
    try:
        ix = sa.DeviceIndex(t, arr)
        for cap in (5, 70):
            ml, pos = match_model(t, arr, q, cap)
            for want in _WANTS:
                got = host_call(ix, q, cap, want)
                assert (not want[0] or np.array_equal(got[0], ml)) and (not want[1] or np.array_equal(got[1], pos))
                check_stats(ml, q.size, t.size, cap, lanes=lanes)
                if want == (True, True):
                    same_for_every_width(("offsets", cap), lanes, *got)
                for off in range(8):
                    dev = stats_on_device(ix, q, cap, off, want)
                    assert (not want[0] or np.array_equal(dev[0], ml)) and (not want[1] or np.array_equal(dev[1], pos)), (cap, want, off)
                    check_stats(ml, q.size, t.size, cap, lanes=lanes)
        ix.close()
    finally:
        sa.match_set_group_lanes(prev)


def _table_texts(oracle):
    out = {"zeros_then_ffs": _u8(_CASES["zeros_ffs"]), "mix00ff": _u8(_CASES["mix00ff"]), "english": corpus.english_corpus(5000, 8),
           "fib": _u8(_CASES["fib"]), "banana": _u8(b"banana"), "empty": _u8(b"")}
    return {k: (v, oracle.sais(v)) for k, v in out.items()}


@pytest.mark.parametrize("lanes", LANES)
def test_answers_do_not_depend_on_the_tables(oracle, lanes):
    prev = sa.match_set_group_lanes(lanes)
    try:
        for name, (t, arr) in _table_texts(oracle).items():
            qs = queries(t, 3)
            qs["edge"] = _u8(b"\x00\x01\x00\xff\xfe\xff\xff\x00\x00" * 30)       # windows whose bigram bucket is empty
            for tables in ((), ("bkt",), ("lcp",), ("bkt", "lcp")):
                ix = sa.DeviceIndex(t, arr)
                if "bkt" in tables:
                    ix.buckets()
                if "lcp" in tables:
                    ix.enable_lcp()
                for qname, q in qs.items():
                    for cap in (1, 2, 3, 9, 65, 300):
                        ml, pos = match_model(t, arr, q, cap)
                        got = host_call(ix, q, cap)
                        assert np.array_equal(got[0], ml) and np.array_equal(got[1], pos), (name, tables, qname, cap)
                        st = check_stats(ml, q.size, t.size, cap, lanes=lanes)
                        assert st["route_long"] == (1 if "lcp" in tables else 0)
                        same_for_every_width(("tables", name, tables, qname, cap), lanes, *got)
                    for k in (1, 2, 5):
                        sp = ix.match_spans(q, k)
                        assert np.array_equal(sp, spans_model(t, arr, q, k)[0]), (name, tables, qname, k)
                        same_for_every_width(("tables", name, tables, qname, "spans", k), lanes, sp)
                ix.close()
    finally:
        sa.match_set_group_lanes(prev)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("group_cap", [0, 8, 64, 5000, -1])
def test_group_cap_routes(oracle, group_cap, lanes):
    eff = 64 if group_cap < 0 else group_cap
    sa.match_set_group_cap(3)
    prev = sa.match_set_group_cap(group_cap)                          # (-1: a cap restored with a negative value)
    assert prev == 3
    prev_lanes = sa.match_set_group_lanes(lanes)
    try:
        for name, (t, arr) in _table_texts(oracle).items():
            for tables in ((), ("bkt", "lcp")):
                ix = sa.DeviceIndex(t, arr)
                if tables:
                    ix.buckets()
                    ix.enable_lcp()
                for qname in ("same", "changed", "random", "m257"):
                    q = queries(t, 5)[qname]
                    for cap in (1, 7, 8, 9, 64, 65, 4096, 6000):
                        ml, pos = match_model(t, arr, q, cap)
                        got = host_call(ix, q, cap)
                        assert np.array_equal(got[0], ml) and np.array_equal(got[1], pos), (name, tables, qname, cap)
                        st = check_stats(ml, q.size, t.size, cap, eff, lanes=lanes)
                        if qname == "same" and cap > min(eff, STAGE_MAX) and t.size > cap:
                            assert st["long_positions"] > 0
                        same_for_every_width(("group_cap", group_cap, name, tables, qname, cap), lanes, *got)
                    k = 50
                    sp = spans_model(t, arr, q, k)
                    got = ix.match_spans(q, k)
                    assert np.array_equal(got, sp[0])
                    check_stats(match_model(t, arr, q, k)[0], q.size, t.size, k, eff, spans=sp, lanes=lanes)
                    same_for_every_width(("group_cap", group_cap, name, tables, qname, "spans"), lanes, got)
                ix.close()
    finally:
        sa.match_set_group_cap(-1)
        sa.match_set_group_lanes(prev_lanes)


def test_work_bound_one_byte_text():
    n, m, cap = 1 << 16, 1 << 14, 4096
    t = np.full(n, 0x41, dtype=np.uint8)
    arr = np.arange(n, -1, -1, dtype=np.uint32)
    q = np.full(m, 0x41, dtype=np.uint8)
    ml = np.minimum(cap, m - np.arange(m))
    pos = n - ml                                                      # the lower bound of a^c is the suffix a^c itself
    for table in (False, True):
        ix = sa.DeviceIndex(t, arr)
        if table:
            ix.enable_lcp()
        got = ix.match_stats(q, cap)
        assert np.array_equal(got[0], ml) and np.array_equal(got[1], pos)
        st = check_stats(ml, m, n, cap)
        assert st["route_long"] == int(table) and st["long_positions"] == m - 64
        print("one byte", "table" if table else "plain", st["compared_bytes"] / m, "bytes a position")
        ix.close()


def test_work_bound_fibonacci(oracle):
    t = _u8(fibonacci_word(20)[:16000])
    arr = oracle.sais(t)
    q = np.ascontiguousarray(t[1:])
    for table in (False, True):
        ix = sa.DeviceIndex(t, arr)
        if table:
            ix.enable_lcp()
        for cap in (64, 4096):
            got = ix.match_stats(q, cap)
            ml = np.minimum(cap, q.size - np.arange(q.size))
            assert np.array_equal(got[0], ml)
            tb = t.tobytes()
            for j in range(0, q.size, 97):
                assert tb[int(got[1][j]):int(got[1][j]) + int(ml[j])] == tb[j + 1:j + 1 + int(ml[j])]
            st = check_stats(ml, q.size, t.size, cap)
            assert st["route_long"] == int(table)
            print("fibonacci", cap, "table" if table else "plain", st["compared_bytes"] / q.size, "bytes a position")
        ix.close()


def test_spans(oracle):
    for name, (t, arr) in _table_texts(oracle).items():
        ix = sa.DeviceIndex(t, arr)
        s = sa.SuffixArray.unchecked_from_parts(t, arr)
        for qname, q in queries(t, 7).items():
            m = q.size
            for k in (1, 2, 5, 50, max(m, 1), m + 1):
                sp = spans_model(t, arr, q, k)
                got = ix.match_spans(q, k)
                assert got.dtype == np.uint32 and got.shape == sp[0].shape and np.array_equal(got, sp[0]), (name, qname, k)
                check_stats(match_model(t, arr, q, k)[0], m, t.size, k, spans=sp)
                assert np.array_equal(s.match_spans(q, k), sp[0])
                count, dev = spans_on_device(ix, q, k, max((m + 1) // (k + 1), 1), m % 8)
                assert count == sp[0].shape[0] and np.array_equal(dev, sp[0]), (name, qname, k)
        ix.close()


def test_span_capacity(oracle):
    t = corpus.english_corpus(9000, 12)
    arr = oracle.sais(t)
    q = queries(corpus.english_corpus(6000, 13), 1)["same"]
    k = 4
    sp = spans_model(t, arr, q, k)
    z = sp[0].shape[0]
    assert z > 8
    ix = sa.DeviceIndex(t, arr)
    ml = match_model(t, arr, q, k)[0]
    for cap in (0, 1, z - 1, z, z + 1):
        count, dev = spans_on_device(ix, q, k, cap)
        assert count == z and np.array_equal(dev, sp[0][:cap]), cap
        check_stats(ml, q.size, t.size, k, spans=sp)
    out = np.full((5, 2), 0xEEEEEEEE, dtype=np.uint32)
    cnt = ctypes.c_int64(0)
    assert sa.lib().sa_amd_index_match_spans(ix._h, q.ctypes.data, q.size, k, out.ctypes.data, 3, ctypes.byref(cnt)) == 0
    assert cnt.value == z and np.array_equal(out[:3], sp[0][:3]) and np.all(out[3:] == 0xEEEEEEEE)
    check_stats(ml, q.size, t.size, k, spans=sp)
    ix.close()


def test_errors():
    L = sa.lib()
    t, q = _u8(b"mississippi"), _u8(b"missing pips")
    m = q.size
    ix = sa.DeviceIndex(t)
    out = np.full(4 * m, 0x77777777, dtype=np.uint32)
    o = out.ctypes.data
    cnt = ctypes.c_int64(-5)
    c = ctypes.byref(cnt)
    assert L.sa_amd_index_match_stats(None, q.ctypes.data, m, 4, o, o) == -1
    assert L.sa_amd_index_match_stats(ix._h, q.ctypes.data, -1, 4, o, o) == -1
    assert L.sa_amd_index_match_stats(ix._h, None, m, 4, o, o) == -1
    assert L.sa_amd_index_match_stats(ix._h, q.ctypes.data, m, 0, o, o) == -1
    assert L.sa_amd_index_match_spans(ix._h, q.ctypes.data, m, 0, o, m, c) == -1
    assert L.sa_amd_index_match_spans(ix._h, q.ctypes.data, m, 2, o, -1, c) == -1
    assert L.sa_amd_index_match_spans(None, q.ctypes.data, m, 2, o, m, c) == -1
    assert cnt.value == -5 and np.all(out == 0x77777777)
    with pytest.raises(ValueError):
        ix.match_stats(q, 0)
    with pytest.raises(ValueError):
        ix.match_spans(q, 0)
    wb = sa.match_work_bytes(m)
    with _Dev(m, 8 * m + 512, wb + 256) as d:
        dQ, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * m + 512) == 0
        assert d.hip.hipMemcpy(dQ, q.ctypes.data, m, 1) == 0
        assert L.sa_amd_index_match_stats_device(ix._h, dQ, m, 4, dO, dO + 4 * m, dW, 64, None) == -1           # short work block
        assert L.sa_amd_index_match_stats_device(ix._h, dQ, m, 4, dO, dO + 4 * m, dW + 4, wb, None) == -1       # misaligned work block
        assert L.sa_amd_index_match_stats_device(ix._h, dQ, m, 0, dO, dO + 4 * m, dW, wb, None) == -1
        assert L.sa_amd_index_match_stats_device(ix._h, None, m, 4, dO, dO + 4 * m, dW, wb, None) == -1
        assert L.sa_amd_index_match_stats_device(ix._h, dQ, -1, 4, dO, dO + 4 * m, dW, wb, None) == -1
        assert L.sa_amd_index_match_stats_device(None, dQ, m, 4, dO, dO + 4 * m, dW, wb, None) == -1
        assert L.sa_amd_index_match_spans_device(ix._h, dQ, m, 2, dO, m, c, dW + 128, wb, None) == -1
        assert L.sa_amd_index_match_spans_device(ix._h, dQ, m, 2, dO, m, c, dW, wb - 256, None) == -1
        assert L.sa_amd_index_match_spans_device(ix._h, dQ, m, 2, dO, -1, c, dW, wb, None) == -1
        assert L.sa_amd_index_match_spans_device(ix._h, dQ, m, 0, dO, m, c, dW, wb, None) == -1
        raw = np.zeros(8 * m + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
        assert np.all(raw == CANARY) and cnt.value == -5
        assert L.sa_amd_index_match_spans_device(ix._h, dQ, m, 2, dO, m, c, dW, wb, None) == 0 and cnt.value == ix.match_spans(q, 2).shape[0]
    ix.close()


def test_wrong_permutation_stays_in_bounds():
    """entries in range that are no suffix array: unspecified answers, but the canaries hold and the call ends"""
    rng = np.random.default_rng(78)
    n = 20000
    t = corpus.english_corpus(n, 2)
    arr = np.empty(n + 1, dtype=np.uint32)
    arr[0] = n
    arr[1:] = rng.integers(0, n + 1, n)
    q = queries(t, 4)["changed"][:5000]
    for tables in (False, True):
        ix = sa.DeviceIndex(t, arr)
        if tables:
            ix.buckets()
        for cap in (3, 64, 500):
            got = stats_on_device(ix, q, cap, 3)
            assert np.all(got[0] <= cap)
        ix.close()


# ---------------------------------------------------------------- a million bytes, exact ----
# match_definition is a Python loop and stops at some ten thousand bytes; oracle_match_stats (oracle/oracle.c) restates the
# header on host threads.  At this size the bigram buckets of both texts are well filled (the table's starts matter), a query
# sends tens of thousands of positions down the long path and the descent over the LCP table runs at log_p = 21.
MID_N = (1 << 20) + 3
MID_M = (1 << 16) + 77
MID_ABSENT = 2000
_MID = {}


def mid_case(oracle, name):
    """(text, array, query, {cap: (ML, POS)}) computed once and left unchanged"""
    if name in _MID:
        return _MID[name]
    t = corpus.english_corpus(MID_N, 21) if name == "english" else corpus.dna(MID_N, 22)
    arr = oracle.sais(t)
    rng = np.random.default_rng(23)
    parts, have = [], 0
    while have < MID_M - MID_ABSENT:                                 # slices of the text, 1 .. 6000 bytes, from anywhere in it
        ln = int(min(rng.integers(1, 6001), MID_M - MID_ABSENT - have))
        at = int(rng.integers(0, MID_N - ln + 1))
        parts.append(t[at:at + ln])
        have += ln
    q = np.concatenate(parts)
    flips = rng.choice(q.size, q.size // 37, replace=False)           # one byte in 37, wherever it falls: the gaps between two
    q[flips] ^= 1                                                     # changed bytes run from nothing to some hundred bytes
    absent = np.setdiff1d(np.arange(256, dtype=np.uint8), np.unique(t))
    half = q.size // 2 + 1
    q = np.ascontiguousarray(np.concatenate([q[:half], np.full(MID_ABSENT, absent[0], dtype=np.uint8), q[half:]]))
    assert q.size == MID_M and t.size == MID_N
    exact = {cap: oracle_match_stats(oracle, t, arr, q, cap) for cap in MID_CAPS + (50,)}
    for a in (t, arr, q) + tuple(x for pair in exact.values() for x in pair):
        a.flags.writeable = False
    _MID[name] = (t, arr, q, exact)
    return _MID[name]


MID_CAPS = (1, 2, 3, 64, 65, 300, 4096, MID_M + 5)


@pytest.mark.parametrize("tables", [(), ("bkt",), ("lcp",), ("bkt", "lcp")], ids=["plain", "bkt", "lcp", "bkt_lcp"])
@pytest.mark.parametrize("name", ["english", "dna"])
def test_mid_size_exact(oracle, name, tables):
    t, arr, q, exact = mid_case(oracle, name)
    n, m = t.size, q.size
    ix = sa.DeviceIndex(t, arr)
    if "bkt" in tables:
        ix.buckets()
    if "lcp" in tables:
        ix.enable_lcp()
    for turn, cap in enumerate(MID_CAPS):
        ml, pos = exact[cap]
        got = host_call(ix, q, cap)
        assert np.array_equal(got[0], ml), (name, tables, cap, np.flatnonzero(got[0] != ml)[:8])
        assert np.array_equal(got[1], pos), (name, tables, cap, np.flatnonzero(got[1] != pos)[:8])
        st = check_stats(ml, m, n, cap, lanes=8)
        assert st["long_positions"] == long_positions_definition(ml, m, cap, 64)
        assert (st["long_positions"] > 0) == (cap > 64), (cap, st)
        assert st["route_long"] == (1 if "lcp" in tables else 0)
        if cap > 64:
            print(name, tables, "cap", cap, "long positions", st["long_positions"], "bytes a position", st["compared_bytes"] / m)
        dev = stats_on_device(ix, q, cap, 1 + 2 * (turn % 4))        # an odd byte address for the query
        assert np.array_equal(dev[0], ml) and np.array_equal(dev[1], pos), (name, tables, cap)
        assert check_stats(ml, m, n, cap, lanes=8)["long_positions"] == st["long_positions"]
    assert np.all(exact[MID_M + 5][0][q == q[m // 2]] == 0)           # (the absent letter's run sits around the middle)
    k = 50
    ml = exact[k][0]
    flagged = np.flatnonzero(ml == k)
    sp = union_spans(flagged, [k] * flagged.size, m)
    z = sp.shape[0]
    assert z > 64
    for capacity in (z // 2, z):
        count, dev = spans_on_device(ix, q, k, capacity, 3)           # (checks the canaries on either side and behind the spans)
        assert count == z and np.array_equal(dev, sp[:capacity]), (name, tables, capacity)
        check_stats(ml, m, n, k, spans=(sp, flagged), lanes=8)
    assert np.array_equal(ix.match_spans(q, k), sp)
    ix.close()


def _brute_region(region, qb):
    """longest prefix of every qb[j:] that occurs in region, by bytes.find (the answer at j + 1 is at least the one at j, less 1)"""
    out, ln = [], 0
    for j in range(len(qb)):
        ln = max(ln - 1, 0)
        while j + ln < len(qb) and region.find(qb[j:j + ln + 1]) >= 0:
            ln += 1
        out.append(ln)
    return np.array(out, dtype=np.int64)


def test_top_of_the_range():
    n = N_ABOVE
    t = corpus.dna(n, 41)
    ix = sa.DeviceIndex(t)                                            # the array is built on the device and stays there
    rng = np.random.default_rng(9)
    m = 8192
    start = n - m - 7                                                 # the second half of the query lies above 2^30
    q = t[start:start + m].copy()
    assert 0x4E not in np.unique(t[:1 << 20])
    q[rng.integers(0, m, 40)] = 0x4E                                  # 'N': not a byte of the text
    tail = t[n - 65536:].tobytes()
    qb = q.tobytes()
    ml, pos = ix.match_stats(q, m + 5)
    ml, pos = ml.astype(np.int64), pos.astype(np.int64)
    st = sa.last_match_stats()
    assert np.all(ml >= _brute_region(tail, qb))                      # the text holds at least what its last 64 KiB hold
    assert np.all(ml[1:] >= ml[:-1] - 1) and np.all(ml <= m - np.arange(m))
    assert np.all(ml[q == 0x4E] == 0) and np.all(pos[ml == 0] == NONE)
    on = np.flatnonzero(ml > 0)
    assert np.all(pos[on] + ml[on] <= n) and np.count_nonzero(pos[on] > 1 << 30) > m // 4    # the long matches lie where the query was cut
    for j in on:
        assert t[pos[j]:pos[j] + ml[j]].tobytes() == qb[j:j + ml[j]], j
        assert pos[j] + ml[j] == n or j + ml[j] == m or t[pos[j] + ml[j]] != q[j + ml[j]]
    assert st["longest"] == int(ml.max()) and st["ml_sum"] == int(ml.sum()) and st["long_positions"] > 0
    cap = 64
    ml2, pos2 = ix.match_stats(q, cap)
    assert np.array_equal(ml2, np.minimum(ml, cap))
    pin_to_search(ix, q, cap, ml2.astype(np.int64), pos2.astype(np.int64))
    sp = ix.match_spans(q, 50).astype(np.int64)
    cover = np.zeros(m + 1, dtype=np.int64)
    keep = np.flatnonzero(ml >= 50)
    np.add.at(cover, keep, 1)
    np.add.at(cover, keep + ml[keep], -1)
    inside = np.zeros(m, dtype=bool)
    for a, b in sp:
        inside[a:b] = True
    assert np.array_equal(inside, np.cumsum(cover)[:m] > 0)
    ix.close()
    del t
    sa.lib().sa_amd_release_cache()


def test_thread_safety(oracle):
    t = corpus.english_corpus(12000, 30)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    ix.buckets()
    qs = [queries(corpus.english_corpus(3000 + 100 * j, 31 + j), j)["same"] for j in range(2)]
    exp = [(match_model(t, arr, q, 40), spans_model(t, arr, q, 6)) for q in qs]
    errors = []

    def work(j):
        try:
            for _ in range(4):
                got = ix.match_stats(qs[j], 40)
                st = sa.last_match_stats()
                assert np.array_equal(got[0], exp[j][0][0]) and np.array_equal(got[1], exp[j][0][1])
                check_stats(exp[j][0][0], qs[j].size, t.size, 40, st=st)
                assert np.array_equal(ix.match_spans(qs[j], 6), exp[j][1][0])
                assert sa.last_match_stats()["spans"] == exp[j][1][0].shape[0]
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    ix.close()
