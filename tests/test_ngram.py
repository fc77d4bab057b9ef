"""GPU suite for the n-gram / infinity-gram queries of the device index: next_bytes and infgram compared bit for bit with the
definitions of tests/test_ngram_abi.py (numpy over the oracle's suffix array, checked against brute force there), canaries
around every output, the statistics with that file's models of the routes and of the bisection.

Sizes: texts from 0 bytes to 1 MiB; every index of these kernels is 64-bit or bounded by n + 1 < 2^31."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT
from test_docs import same_for_every_route, some_patterns
from test_docs_abi import _u8
from test_ngram_abi import (EXAMPLE_TEXT, backoff_bound, backoff_cap, ceil_log2, infgram_definition, listing_of, next_bytes_definition,
                            route_of, search_route_bound)

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
PAD = 32
PER_PATTERN = ("suffix_len", "lo", "hi", "at_end")
HUGE = 1 << 30
CAPS = (0, 64, -1, HUGE)


def raw_call(ix, pats, capacity, backoff=None, null=()):
    """sa_amd_index_next_bytes (backoff=None) or sa_amd_index_infgram (backoff=(min_count, max_len)) on numpy buffers with canaries
    around every output; the outputs named in `null` are passed as NULL -> dict of what was written (None for a NULL output)"""
    data, off, cnt = sa._pattern_batch(pats)
    room = min(capacity, 1 << 22)
    bufs = {"suffix_len": np.full(cnt + 2 * PAD, FILL32, dtype=np.uint32), "lo": np.full(cnt + 2 * PAD, FILL32, dtype=np.uint32),
            "hi": np.full(cnt + 2 * PAD, FILL32, dtype=np.uint32), "at_end": np.full(cnt + 2 * PAD, 0xA5, dtype=np.uint8),
            "list_off": np.full(cnt + 1 + 2 * PAD, -7, dtype=np.int64), "bytes": np.full(room + 2 * PAD, 0xA5, dtype=np.uint8),
            "counts": np.full(room + 2 * PAD, FILL32, dtype=np.uint32)}
    fill = {k: v[0].copy() for k, v in bufs.items()}

    def ptr(name):
        return None if name in null else bufs[name][PAD:].ctypes.data
    total = ctypes.c_int64(-1)
    tp = None if "total" in null else ctypes.byref(total)
    if backoff is None:
        rc = sa.lib().sa_amd_index_next_bytes(ix._h, data.ctypes.data, off.ctypes.data, cnt, ptr("lo"), ptr("hi"), ptr("at_end"), ptr("list_off"),
                                              ptr("bytes"), ptr("counts"), capacity, tp)
    else:
        rc = sa.lib().sa_amd_index_infgram(ix._h, data.ctypes.data, off.ctypes.data, cnt, backoff[0], backoff[1], ptr("suffix_len"), ptr("lo"),
                                           ptr("hi"), ptr("at_end"), ptr("list_off"), ptr("bytes"), ptr("counts"), capacity, tp)
    assert rc == 0, rc
    st = sa.last_ngram_stats()
    listed = st["entries"]
    if "total" not in null:
        assert total.value == listed
    wrote = min(listed, capacity)
    extent = {name: cnt for name in PER_PATTERN}
    extent.update(list_off=cnt + 1, bytes=wrote, counts=wrote)
    if backoff is None:
        extent["suffix_len"] = 0
    out = {"total": listed, "stats": st}
    for name, buf in bufs.items():                                    # nothing before, nothing past what fits, nothing at all through NULL
        k = 0 if name in null else extent[name]
        assert np.all(buf[:PAD] == fill[name]) and np.all(buf[PAD + k:] == fill[name]), name
        out[name] = None if name in null or (backoff is None and name == "suffix_len") else buf[PAD:PAD + k].copy()
    return out


def expected_listing(exp):
    """exp: per pattern (lo, hi, at_end, next) -> (list_off, bytes, counts) of the whole batch"""
    pairs = [listing_of(e[3]) for e in exp]
    loff = np.concatenate([[0], np.cumsum([b.size for b, _ in pairs])]).astype(np.int64)
    return loff, np.concatenate([b for b, _ in pairs] + [np.zeros(0, np.uint8)]), np.concatenate([c for _, c in pairs] + [np.zeros(0, np.uint32)])


def effective_cap(cap):
    return sa.NGRAM_STREAM_CAP_DEFAULT if cap < 0 else min(cap, 2**31 - 1)


def check_outputs(got, exp, what):
    loff, b, c = expected_listing(exp)
    assert got["total"] == loff[-1], what
    assert np.array_equal(got["lo"], [e[0] for e in exp]) and np.array_equal(got["hi"], [e[1] for e in exp]), what
    assert np.array_equal(got["at_end"], [e[2] for e in exp]), what
    assert np.array_equal(got["list_off"], loff) and np.array_equal(got["bytes"], b) and np.array_equal(got["counts"], c), what
    for q, e in enumerate(exp):                                       # the header's identity on the device's own numbers
        assert int(got["counts"][loff[q]:loff[q + 1]].sum()) + int(got["at_end"][q]) == int(got["hi"][q]) - int(got["lo"][q])


def check_route_stats(st, exp, cap, backoff):
    eff = effective_cap(cap)
    cnts = [e[1] - e[0] - e[2] for e in exp]
    routes = [route_of(c, eff) for c in cnts]
    want = {"patterns": len(exp), "stream_slots": sum(c for c, r in zip(cnts, routes) if r == "stream"),
            "stream_queries": routes.count("stream"), "search_queries": routes.count("search"), "empty_queries": routes.count("empty"),
            "entries": int(sum(np.count_nonzero(e[3]) for e in exp)), "stream_cap": eff, "readbacks": 1, "backoff": int(backoff)}
    assert {f: st[f] for f in want} == want, (st, want)
    assert 64 * routes.count("search") <= st["search_slots"] <= sum(search_route_bound(c) for c, r in zip(cnts, routes) if r == "search")


def check_next(ix, exp, pats, cap=-1, key=None, route=None):
    """next_bytes and its statistics against the definitions' answers `exp`"""
    prev = sa.ngram_set_stream_cap(cap)
    try:
        got = raw_call(ix, pats, int(sum(np.count_nonzero(e[3]) for e in exp)) + 5)
    finally:
        sa.ngram_set_stream_cap(prev)
    check_outputs(got, exp, (cap, route))
    st = got["stats"]
    check_route_stats(st, exp, cap, False)
    assert (st["range_searches"], st["compared_bytes"], st["passes"]) == (len(pats), -1, 2)
    if key is not None:
        same_for_every_route(key, route, got["lo"], got["hi"], got["at_end"], got["list_off"], got["bytes"], got["counts"])
    return got


def check_inf(ix, tb, arr, prompts, min_count=1, max_len=0, cap=-1, key=None, route=None):
    """infgram and its statistics against the definition; every s cross-checked with the index's own search"""
    defs = [infgram_definition(tb, arr, p, min_count, max_len) for p in prompts]
    exp = [d[1:5] for d in defs]
    prev = sa.ngram_set_stream_cap(cap)
    try:
        got = raw_call(ix, prompts, int(sum(np.count_nonzero(e[3]) for e in exp)) + 5, backoff=(min_count, max_len))
    finally:
        sa.ngram_set_stream_cap(prev)
    assert np.array_equal(got["suffix_len"], [d[0] for d in defs]), (min_count, max_len, route)
    check_outputs(got, exp, (min_count, max_len, cap, route))
    st = got["stats"]
    check_route_stats(st, exp, cap, True)
    caps = [backoff_cap(len(p), max_len) for p in prompts]
    assert st["range_searches"] <= sum(ceil_log2(c + 1) for c in caps) <= sum(backoff_bound(c) for c in caps)
    assert st["range_searches"] >= sum(1 for c in caps if c >= 1) and st["compared_bytes"] >= 0 and st["passes"] == 2
    # the suffix of s bytes qualifies under DeviceIndex.search, the one of s + 1 bytes, where the cap allows it, does not
    s = got["suffix_len"].astype(np.int64)
    r = ix.search([p[len(p) - int(k):] if k else b"" for p, k in zip(prompts, s)])
    assert np.array_equal(r["lo"], got["lo"]) and np.array_equal(r["hi"], got["hi"])
    assert all(k == 0 or int(h) - int(l) >= min_count for k, l, h in zip(s, r["lo"], r["hi"]))
    longer = [(p, int(k) + 1) for p, k, c in zip(prompts, s, caps) if k < c]
    if longer:
        r = ix.search([p[len(p) - k:] for p, k in longer])
        assert np.all(r["hi"].astype(np.int64) - r["lo"].astype(np.int64) < min_count)
    if key is not None:
        same_for_every_route(key, route, got["suffix_len"], got["lo"], got["hi"], got["at_end"], got["list_off"], got["bytes"], got["counts"])
    return got


def contexts_of(tb):
    """the empty context, every single byte, absent contexts, suffixes of the text, the whole text and the whole text plus a byte"""
    n = len(tb)
    pats = [b""] + [bytes([b]) for b in range(256)] + [b"\x01\x02nope", b"zq\x00zq"]
    pats += [tb[n - k:] for k in (1, 2, 3, 5, 64, 65, 130) if k <= n]
    return pats + [tb, tb + b"a", tb + b"\x00"] + (some_patterns(tb, n + 3, 12) if n else [])


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
        tb = f.read()
    return tb, np.fromfile(os.path.join(ROOT, "tests", "golden", name + ".sa.u32le"), dtype="<u4")


@functools.lru_cache(maxsize=None)
def big_text(kind):
    """-> (text bytes, suffix array): computed once, shared, never changed"""
    if kind == "sigma4_64k":
        t = (np.random.default_rng(4).integers(0, 4, 1 << 16) + 97).astype(np.uint8)
    elif kind == "english_1m":
        t = corpus.english_corpus(1 << 20, 11)
    else:
        t = corpus.english_corpus(int(kind), 5)
    from conftest import Oracle
    arr = Oracle().sais(t)
    arr.setflags(write=False)
    return t.tobytes(), arr


def expected(tb, arr, pats):
    memo = {}
    for p in pats:
        if p not in memo:
            memo[p] = next_bytes_definition(tb, arr, p)
    return [memo[p] for p in pats]


# ---------------------------------------------------------------- next_bytes ----

def test_known_answers():
    t = _u8(EXAMPLE_TEXT)
    ix = sa.DeviceIndex(t)                                             # the array is built on the device
    lo, hi, ae, loff, b, c = ix.next_bytes([b"a", b"abra", b"", b"x"])
    assert (lo.tolist(), hi.tolist(), ae.tolist()) == ([1, 2, 0, lo[3]], [6, 4, 12, lo[3]], [1, 1, 1, 0])
    assert loff.tolist() == [0, 3, 4, 9, 9] and bytes(b) == b"bcdcabcdr" and c.tolist() == [2, 1, 1, 1, 5, 2, 1, 1, 2]
    assert (b.dtype, c.dtype, lo.dtype, ae.dtype, loff.dtype) == (np.uint8, np.uint32, np.uint32, np.uint8, np.int64)
    dlo, dhi, dae, nxt = ix.next_bytes([b"a", b"abra", b"", b"x"], dense=True)
    assert nxt.shape == (4, 256) and nxt.dtype == np.uint32 and np.array_equal(dlo, lo) and np.array_equal(dae, ae)
    assert {chr(k): int(v) for k, v in enumerate(nxt[2]) if v} == {"a": 5, "b": 2, "c": 1, "d": 1, "r": 2} and not nxt[3].any()
    for (min_count, max_len), want in (((1, 0), (4, 2, 4)), ((2, 0), (4, 2, 4)), ((3, 0), (1, 1, 6)), ((1, 2), (2, 10, 12))):
        s, lo, hi, ae, loff, b, c = ix.infgram([b"xcabra"], min_count, max_len)
        assert (int(s[0]), int(lo[0]), int(hi[0])) == want and ae[0] == 1
    assert bytes(ix.infgram([b"xcabra"], 3)[5]) == b"bcd"
    assert ix.next_bytes([])[3].tolist() == [0] and ix.infgram([])[4].tolist() == [0]
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram([b"a"], 0)
    ix.close()
    s = sa.SuffixArray(t)                                              # the same two on the lazily made index
    assert s.next_bytes([b"abra"])[5].tolist() == [1] and int(s.infgram([b"xcabra"], 3)[0][0]) == 1


@pytest.mark.parametrize("tb", [b"", b"a", b"banana", b"mississippi", EXAMPLE_TEXT], ids=["n0", "n1", "banana", "mississippi", "abracadabra"])
def test_small_texts(oracle, tb):
    t = _u8(tb)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    pats = contexts_of(tb)
    exp = expected(tb, arr, pats)
    if not tb:
        assert exp[0][:3] == (0, 1, 1) and not exp[0][3].any()         # n = 0: the range [0, 1), at_end, an empty listing
    for cap in CAPS:
        check_next(ix, exp, pats, cap, key=("small", tb), route=cap)
    for min_count in (1, 2, 3, len(tb) + 1, len(tb) + 2):
        check_inf(ix, tb, arr, [b"", b"q", tb, tb + b"a", b"x" + tb, tb[1:], b"ssi", b"xcabra", b"ana"], min_count)
    ix.close()


@pytest.mark.parametrize("name", ["all_bytes_twice", "a_run_1025", "zeros_then_ffs", "fibonacci_15", "thue_morse_2k"])
def test_golden_texts(name):
    tb, arr = golden(name)
    ix = sa.DeviceIndex(_u8(tb), arr)
    pats = contexts_of(tb)
    if name == "a_run_1025":
        pats += [b"a" * k for k in (2, 63, 64, 65, 1024, 1025, 1026)]
    exp = expected(tb, arr, pats)
    if name == "all_bytes_twice":
        assert np.count_nonzero(exp[0][3]) == 256                       # every continuation of the empty context is present
    if name == "a_run_1025":
        assert all(e[2] == 1 and np.count_nonzero(e[3]) == (1 if p != tb else 0) for e, p in zip(exp, pats) if p and set(p) == {97} and len(p) <= 1025)
    for cap in CAPS:
        check_next(ix, exp, pats, cap, key=("golden", name), route=cap)
    check_inf(ix, tb, arr, [tb[5:40], tb[-9:], b"\x07" + tb[:33], tb], 2)
    ix.close()


def test_range_sizes_around_the_wave_and_the_cap(oracle):
    """contexts whose stripped range has exactly 0, 1, 63, 64, 65, 127, 128, 129, 255, 256 and 257 slots"""
    sizes = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
    tb = b"".join(bytes([200, j, 1 + i % 7]) for j, c in enumerate(sizes) for i in range(c)) + b"\xc8\xf0"
    t = _u8(tb)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    pats = [bytes([200, j]) for j in range(len(sizes))] + [b"\xc8\xf0", b"\xc8\xf1"]       # the last two: a suffix (1 slot, at_end), absent
    exp = expected(tb, arr, pats)
    assert [e[1] - e[0] - e[2] for e in exp] == list(sizes) + [0, 0] and [e[1] - e[0] for e in exp][-2:] == [1, 0]
    for cap in (-1, 0, 63, 64, 65, 256, HUGE):
        got = check_next(ix, exp, pats, cap, key="sizes", route=cap)
        eff = effective_cap(cap)
        assert got["stats"]["stream_queries"] == sum(1 for c in sizes if c <= eff)
    ix.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 70000])
def test_batch_sizes(count):
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    pool = some_patterns(tb, 31, 400) + [b"e", b" ", b"th", tb[-3:]]
    pats = [pool[(7 * q) % len(pool)] for q in range(count)]
    exp = expected(tb, arr, pats)
    check_next(ix, exp, pats)
    if count == 70000:
        check_next(ix, exp, pats, 0)
    ix.close()


@pytest.mark.parametrize("tables", [(), ("bkt",), ("lcp",), ("bkt", "lcp")], ids=["plain", "bkt", "lcp", "bkt_lcp"])
def test_answers_do_not_depend_on_the_route(tables):
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    if "bkt" in tables:
        ix.buckets()
    if "lcp" in tables:
        ix.enable_lcp()
    pats = contexts_of(tb)
    exp = expected(tb, arr, pats)
    prompts = some_patterns(tb, 8, 20) + [tb[100:400], tb[100:399] + b"\x00", b"\x00" + tb[500:520], tb[-40:], b"e", b"q\x00"]
    for cap in CAPS:
        check_next(ix, exp, pats, cap, key="next_routes", route=(tables, cap))
        check_inf(ix, tb, arr, prompts, 2, 0, cap, key="inf_routes", route=(tables, cap))
    ix.close()


@pytest.mark.parametrize("kind", ["sigma4_64k", "english_1m"])
def test_large_texts(kind):
    """ranges above 65 536 slots: the empty context of the 64 KiB text (65 537 slots; its single bytes hold a quarter each) and
    the frequent single bytes of the 1 MiB text"""
    tb, arr = big_text(kind)
    ix = sa.DeviceIndex(_u8(tb), arr)
    pats = [b""] + [bytes([b]) for b in sorted(set(tb))] + some_patterns(tb, 12, 20) + [tb[-2:], b"\xfe"]
    exp = expected(tb, arr, pats)
    assert max(e[1] - e[0] for e in exp[1:]) > (65536 if kind == "english_1m" else 16000) and exp[0][1] - exp[0][0] > 65536
    for cap in CAPS:
        check_next(ix, exp, pats, cap, key=("large", kind), route=cap)
    check_inf(ix, tb, arr, [tb[1000:1256], tb[5000:5255] + b"\x00", tb[7000:7100] + b"\x00" + tb[9000:9050]], 1, 0)
    ix.close()


# ---------------------------------------------------------------- back-off ----

def test_backoff_lengths_counts_and_caps():
    tb, arr = big_text("30000")
    n = len(tb)
    ix = sa.DeviceIndex(_u8(tb), arr)
    base = tb[4000:4200]
    prompts = [b"", b"\x00\x01\x02", base]                              # s = 0 twice, s = L
    for d in range(71):                                                # one substituted byte d bytes before the end: s across the 64-byte chunk
        p = bytearray(base)
        p[len(p) - 1 - d] = 0
        prompts.append(bytes(p))
    got = check_inf(ix, tb, arr, prompts, 1, 0)
    assert got["suffix_len"][:3].tolist() == [0, 0, len(base)] and got["suffix_len"][3:].tolist() == list(range(71))
    for min_count in (2, 3, n + 1, n + 2):
        got = check_inf(ix, tb, arr, prompts, min_count, 0)
        if min_count > n:
            assert not got["suffix_len"].any() and np.all(got["hi"] == n + 1)
    some = [prompts[2], prompts[3], prompts[3 + 40], prompts[3 + 64], prompts[3 + 65]]
    for p in some:
        s = infgram_definition(tb, arr, p, 1, 0)[0]
        for max_len in (0, 1, 2, s - 1, s, s + 1):
            if max_len >= 0:
                check_inf(ix, tb, arr, [p], 1, max_len)
    ix.close()


def test_backoff_prompt_lengths():
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    prompts = [tb[9000:9000 + k] for k in (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 4999, 5000)]
    prompts += [b"\x00" + p for p in prompts] + [p[:len(p) // 2] + b"\x00" + p[len(p) // 2:] for p in prompts]
    for min_count, max_len in ((1, 0), (2, 0), (1, 100)):
        check_inf(ix, tb, arr, prompts, min_count, max_len)
    ix.close()


# ---------------------------------------------------------------- the surface ----

def test_capacity_and_null_outputs():
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    pats = some_patterns(tb, 5, 20) + [b"e", b"", tb[-1:]]
    for backoff in (None, (1, 0)):
        exp = expected(tb, arr, pats) if backoff is None else [infgram_definition(tb, arr, p, 1, 0)[1:5] for p in pats]
        loff, b, c = expected_listing(exp)
        total = int(loff[-1])
        for capacity in (0, total - 1, total, total + 5):
            got = raw_call(ix, pats, capacity, backoff)
            w = min(total, capacity)
            assert got["total"] == total and np.array_equal(got["list_off"], loff)
            assert np.array_equal(got["bytes"], b[:w]) and np.array_equal(got["counts"], c[:w])
            assert got["stats"]["passes"] == (2 if capacity else 1)
        names = ("lo", "hi", "at_end", "list_off", "bytes", "counts", "total") + (("suffix_len",) if backoff else ())
        for name in names:                                             # NULL for every output in turn
            got = raw_call(ix, pats, total + 5, backoff, null=(name,))
            assert got["total"] == total
            for other in names:
                if other not in (name, "total", "suffix_len"):
                    want = {"lo": [e[0] for e in exp], "hi": [e[1] for e in exp], "at_end": [e[2] for e in exp], "list_off": loff, "bytes": b, "counts": c}
                    assert np.array_equal(got[other], want[other]), (name, other)
        got = raw_call(ix, pats, 1 << 62, backoff, null=("bytes", "counts"))      # both NULL: the capacity is ignored
        assert got["total"] == total and np.array_equal(got["list_off"], loff) and got["stats"]["passes"] == 1
        got = raw_call(ix, pats, total, backoff, null=names)            # everything NULL: only the statistics
        assert got["total"] == total
    ix.close()


def test_invalid_arguments_write_nothing():
    t = _u8(EXAMPLE_TEXT)
    ix = sa.DeviceIndex(t)
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    good = np.array([0, 2, 4], dtype=np.int64)
    g = good.ctypes.data
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    before = sa.last_ngram_stats()
    assert L.sa_amd_index_next_bytes(None, p, g, 2, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_infgram(None, p, g, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(ix._h, p, g, -1, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(ix._h, p, g, 2, p, p, p, p, p, p, -1, c) == -1
    assert L.sa_amd_index_infgram(ix._h, p, g, -1, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_infgram(ix._h, p, g, 2, 1, 0, p, p, p, p, p, p, p, -1, c) == -1
    assert L.sa_amd_index_infgram(ix._h, p, g, 2, 0, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_infgram(ix._h, p, g, 2, -1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(ix._h, None, g, 2, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(ix._h, p, None, 2, p, p, p, p, p, p, 4, c) == -1
    for off in bad:
        assert L.sa_amd_index_next_bytes(ix._h, p, off.ctypes.data, 2, p, p, p, p, p, p, 4, c) == -1
        assert L.sa_amd_index_infgram(ix._h, p, off.ctypes.data, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777) and sa.last_ngram_stats() == before
    loff = np.full(3, -7, dtype=np.int64)                              # count == 0 succeeds with list_off[0] = 0
    assert L.sa_amd_index_next_bytes(ix._h, None, None, 0, p, p, p, loff.ctypes.data, p, p, 4, c) == 0
    assert loff.tolist() == [0, -7, -7] and tot.value == 0 and np.all(buf == 0x77777777)
    loff[0], tot.value = -7, -5
    assert L.sa_amd_index_infgram(ix._h, None, None, 0, 1, 0, p, p, p, p, loff.ctypes.data, p, p, 4, c) == 0
    assert loff.tolist() == [0, -7, -7] and tot.value == 0 and np.all(buf == 0x77777777)
    ix.close()


def test_two_threads_query_one_index():
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    batches = [some_patterns(tb, 40 + j, 25) + [b"e", b" ", b""] for j in range(2)]
    exp = [expected(tb, arr, b) for b in batches]
    defs = [[infgram_definition(tb, arr, p, 1, 0) for p in b] for b in batches]
    errors = []

    def work(j):
        try:
            sa.ngram_set_stream_cap(0 if j else 64)                    # (the switch is the calling thread's)
            for _ in range(4):
                got = raw_call(ix, batches[j], 1 << 14)
                check_outputs(got, exp[j], j)
                assert got["stats"]["stream_cap"] == (0 if j else 64) and got["stats"]["patterns"] == len(batches[j])
                inf = raw_call(ix, batches[j], 1 << 14, backoff=(1, 0))
                check_outputs(inf, [d[1:5] for d in defs[j]], j)
                assert np.array_equal(inf["suffix_len"], [d[0] for d in defs[j]])
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.ngram_set_stream_cap(-1) == sa.NGRAM_STREAM_CAP_DEFAULT  # the workers' switches were their own: this thread's is untouched
    ix.close()


def test_the_other_features_statistics_are_left_untouched():
    tb, arr = big_text("30000")
    ix = sa.DeviceIndex(_u8(tb), arr)
    ix.enable_lcp()
    ix.set_documents([0, 1000, len(tb)])
    ix.enable_doc_freq()
    ix.search([b"the", b"e"])
    ix.doc_search([b"the"])
    ix.doc_tf([b"the"])
    readers = (sa.last_search_stats, sa.last_docs_stats, sa.last_doc_tf_stats, sa.last_lcp_stats, sa.last_match_stats, sa.last_stats)
    before = [f() for f in readers]
    ix.next_bytes([b"the", b"", b"e"])
    ix.infgram([tb[50:90], b"q"], 2)
    assert [f() for f in readers] == before
    st = sa.last_ngram_stats()
    assert (st["patterns"], st["backoff"], st["readbacks"]) == (2, 1, 1)
    ix.close()


def test_an_array_that_is_no_suffix_array_is_survived():
    """a permutation of the right entries in the wrong order (every entry in range): the answers are unspecified, but the calls
    return, write inside the outputs only and keep list_off consistent"""
    tb, arr = big_text("30000")
    rng = np.random.default_rng(9)
    s = sa.SuffixArray.unchecked_from_parts(_u8(tb), rng.permutation(arr).astype(np.uint32))
    for tables in ((), ("bkt",)):
        if tables:
            s.enable_buckets()
        ix = s._index()
        pats = contexts_of(tb)
        for cap in (0, -1, HUGE):
            prev = sa.ngram_set_stream_cap(cap)
            try:
                for backoff in (None, (1, 0), (2, 7)):
                    got = raw_call(ix, pats, 300 * len(pats), backoff)
                    loff = got["list_off"]
                    assert loff[0] == 0 and np.all(np.diff(loff) >= 0) and np.all(np.diff(loff) <= 256) and loff[-1] == got["total"]
                    assert np.all(got["hi"] <= len(tb) + 1) and np.all(got["at_end"] <= 1)
            finally:
                sa.ngram_set_stream_cap(prev)
