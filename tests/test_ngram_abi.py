"""CPU suite for the n-gram / infinity-gram queries: the definitions of include/suffix_array_amd.h (at_end, next, the sub-range
identity, the listing, back-off) restated in numpy over the oracle's suffix array and checked against literal brute force on
the raw bytes; pure-Python models of the two continuation routes and of the bisection with their work bounds; the exports, the
Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases
from test_docs_abi import _u8, patterns_of, range_definition

EXPORTS = ("sa_amd_index_next_bytes", "sa_amd_index_infgram", "sa_amd_last_ngram_stats", "sa_amd_ngram_set_stream_cap")
STATS_FIELDS = ("patterns", "range_searches", "compared_bytes", "stream_slots", "search_slots", "stream_queries", "search_queries",
                "empty_queries", "entries", "stream_cap", "readbacks", "backoff", "passes")
EXAMPLE_TEXT = b"abracadabra"
EXAMPLE_SA = [11, 10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2]
WAVE = 64


def ceil_log2(x):
    """ceil(log2(x)) for x >= 1"""
    return (int(x) - 1).bit_length()


# ---------------------------------------------------------------- the definitions ----

def next_bytes_definition(text, arr, pattern):
    """-> (lo, hi, at_end, next): [lo, hi) the slots whose suffix starts with the pattern, at_end = some slot of them has
    SA[i] + p == n, next[b] = the slots with SA[i] + p < n and T[SA[i] + p] == b (256 int64 counts)"""
    t = _u8(text)
    n, p = t.size, len(pattern)
    lo, hi = range_definition(bytes(text), arr, bytes(pattern))
    pos = np.asarray(arr[lo:hi], dtype=np.int64) + p
    at_end = int(np.any(pos == n))
    nxt = np.bincount(t[pos[pos < n]], minlength=256).astype(np.int64)
    return lo, hi, at_end, nxt


def listing_of(nxt):
    """the non-zero (b, next[b]) pairs in ascending b"""
    b = np.flatnonzero(nxt)
    return b.astype(np.uint8), nxt[b].astype(np.uint32)


def backoff_cap(L, max_len):
    return L if max_len <= 0 else min(L, max_len)


def infgram_definition(text, arr, prompt, min_count, max_len):
    """-> (s, lo, hi, at_end, next, probes): s the largest value in 0 .. cap whose suffix of the prompt has at least min_count
    slots; found by the bisection the header allows (the count never grows with s), `probes` range searches"""
    prompt = bytes(prompt)
    L = len(prompt)
    good, bad, probes = 0, backoff_cap(L, max_len) + 1, 0
    while bad - good > 1:
        s = (good + bad) // 2
        lo, hi = range_definition(bytes(text), arr, prompt[L - s:])
        probes += 1
        if hi - lo >= min_count:
            good = s
        else:
            bad = s
    return (good,) + next_bytes_definition(text, arr, prompt[L - good:] if good else b"") + (probes,)


# ---------------------------------------------------------------- the routes' models ----

def stream_route_model(run):
    """the streaming route over the continuation bytes of a stripped range: a slot starts a run where its byte differs from its
    left neighbour's; the counts are the differences of consecutive starts -> (next, slots probed)"""
    run = np.asarray(run, dtype=np.int64)
    start = {}
    for i in np.flatnonzero(np.r_[True, run[1:] != run[:-1]]) if run.size else []:
        start[int(run[i])] = int(i)
    return _counts_of_starts(start, run.size), int(run.size)


def search_route_model(run):
    """the boundary-search route: 64 samples at l (cnt - 1) / 63; between two samples whose bytes differ, every run start is one
    binary search for the first slot above the last byte found -> (next, slots probed)"""
    run = np.asarray(run, dtype=np.int64)
    cnt = int(run.size)
    pos = [(l * (cnt - 1)) // (WAVE - 1) for l in range(WAVE)]
    probes = WAVE
    start = {int(run[0]): 0}
    for l in range(WAVE - 1):
        x, a, bn = int(run[pos[l]]), pos[l], int(run[pos[l + 1]])
        while x < bn:
            u, v, bv = a + 1, pos[l + 1], bn
            while u < v:
                m = u + (v - u) // 2
                probes += 1
                if run[m] > x:
                    v, bv = m, int(run[m])
                else:
                    u = m + 1
            start[bv] = u
            x, a = bv, u
    return _counts_of_starts(start, cnt), probes


def _counts_of_starts(start, cnt):
    nxt = np.zeros(256, dtype=np.int64)
    order = sorted(start)
    for k, b in enumerate(order):
        nxt[b] = (start[order[k + 1]] if k + 1 < len(order) else cnt) - start[b]
    return nxt


def search_route_bound(cnt):
    return 64 + 256 * (ceil_log2(cnt + 1) + 1)


def backoff_bound(cap):
    return 2 * ceil_log2(cap + 1) + 2


def route_of(cnt, stream_cap):
    return "empty" if cnt == 0 else ("stream" if cnt <= stream_cap else "search")


# ---------------------------------------------------------------- brute force ----

def brute_starts(tb, pat, limit=None):
    """every start of an occurrence (the first `limit` of them), overlapping ones included, by bytes.find on the raw bytes; the
    empty pattern occurs at 0 .. n"""
    if not pat:
        return list(range(len(tb) + 1))[:limit]
    out, p = [], tb.find(pat)
    while p >= 0 and (limit is None or len(out) < limit):
        out.append(p)
        p = tb.find(pat, p + 1)
    return out


def brute_next_bytes(tb, pat):
    """-> (occurrences, at_end, next) from the raw bytes alone"""
    starts = brute_starts(tb, pat)
    n, p = len(tb), len(pat)
    nxt = np.zeros(256, dtype=np.int64)
    for s in starts:
        if s + p < n:
            nxt[tb[s + p]] += 1
    return len(starts), int(tb.endswith(pat)), nxt


def brute_infgram(tb, prompt, min_count, max_len):
    """every suffix length tried, longest first"""
    L = len(prompt)
    for s in range(backoff_cap(L, max_len), 0, -1):
        if len(brute_starts(tb, prompt[L - s:], min_count)) >= min_count:
            return s
    return 0


def contexts_of(tb, rng):
    n = len(tb)
    pats = patterns_of(tb, rng, 8) + [tb + b"a", b"\x00", b"\xff"]
    pats += [tb[n - k:] for k in (1, 2, 3, 65) if k <= n]            # suffixes of the text: at_end
    return pats


def prompts_of(tb, rng):
    n = len(tb)
    out = [b"", b"\x01\x02nope"]
    for _ in range(6):
        if n:
            a = int(rng.integers(0, n))
            piece = bytearray(tb[a:a + int(rng.integers(1, 40))])
            out.append(bytes(piece))
            piece[int(rng.integers(0, len(piece)))] ^= 0x55            # one substituted byte: the back-off stops behind it
            out.append(bytes(piece))
    out.append(tb[-7:] if n else b"q")
    return out


def _check_text(tb, oracle, rng):
    n = len(tb)
    arr = oracle.sais(_u8(tb))
    for pat in contexts_of(tb, rng):
        lo, hi, ae, nxt = next_bytes_definition(tb, arr, pat)
        occ, b_ae, b_nxt = brute_next_bytes(tb, pat)
        assert (hi - lo, ae) == (occ, b_ae) and np.array_equal(nxt, b_nxt), pat[:16]
        assert int(nxt.sum()) + ae == hi - lo
        assert ae == 0 or int(arr[lo]) + len(pat) == n                 # only slot lo can be the one at the end
        at = lo + ae
        for b in np.flatnonzero(nxt):                                  # the sub-range of every continuation is the range of c + b
            assert range_definition(tb, arr, pat + bytes([int(b)])) == (at, at + int(nxt[b])), (pat[:16], int(b))
            at += int(nxt[b])
        assert at == hi
        run = _u8(tb)[np.asarray(arr[lo + ae:hi], dtype=np.int64) + len(pat)] if hi > lo + ae else np.zeros(0, dtype=np.uint8)
        assert np.all(np.diff(run.astype(np.int64)) >= 0)              # the stripped range is sorted by the byte behind the context
        got, probed = stream_route_model(run)
        assert np.array_equal(got, nxt) and probed == run.size
        if run.size:
            got, probed = search_route_model(run)
            assert np.array_equal(got, nxt) and probed <= search_route_bound(run.size), pat[:16]
    if n == 0:
        assert next_bytes_definition(tb, arr, b"")[:3] == (0, 1, 1)
    for prompt in prompts_of(tb, rng):
        s0 = None
        for min_count, max_len in ((1, 0), (2, 0), (3, 0), (n + 1, 0), (n + 2, 0), (1, 1), (1, 2), (2, 5), (1, -3)):
            s, lo, hi, ae, nxt, probes = infgram_definition(tb, arr, prompt, min_count, max_len)
            assert s == brute_infgram(tb, prompt, min_count, max_len), (prompt[:16], min_count, max_len)
            cap = backoff_cap(len(prompt), max_len)
            assert probes <= ceil_log2(cap + 1) <= backoff_bound(cap)
            assert s == 0 or hi - lo >= min_count
            if s == 0:
                assert (lo, hi, ae) == (0, n + 1, 1) and np.array_equal(nxt, np.bincount(_u8(tb), minlength=256))
            if (min_count, max_len) == (1, 0):
                s0 = s
        for max_len in (s0 - 1, s0, s0 + 1):                           # the cap around the uncapped answer
            if max_len >= 1:
                assert infgram_definition(tb, arr, prompt, 1, max_len)[0] == min(s0, max_len)


# ---------------------------------------------------------------- the tests ----

def test_the_header_example(oracle):
    tb = EXAMPLE_TEXT
    arr = oracle.sais(_u8(tb))
    assert arr.tolist() == EXAMPLE_SA

    def row(pat):
        lo, hi, ae, nxt = next_bytes_definition(tb, arr, pat)
        b, c = listing_of(nxt)
        return (lo, hi, ae, {chr(x): int(y) for x, y in zip(b, c)})
    assert row(b"a") == (1, 6, 1, {"b": 2, "c": 1, "d": 1})
    assert row(b"abra") == (2, 4, 1, {"c": 1})
    assert row(b"") == (0, 12, 1, {"a": 5, "b": 2, "c": 1, "d": 1, "r": 2})
    lo, hi, ae, nxt = next_bytes_definition(tb, arr, b"x")
    assert lo == hi and ae == 0 and not nxt.any()
    assert infgram_definition(tb, arr, b"xcabra", 1, 0)[:3] == (4, 2, 4)
    assert infgram_definition(tb, arr, b"xcabra", 2, 0)[:3] == (4, 2, 4)
    assert infgram_definition(tb, arr, b"xcabra", 3, 0)[:3] == (1, 1, 6)
    assert infgram_definition(tb, arr, b"xcabra", 1, 2)[:3] == (2, 10, 12)
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    for line in ('"a"       [1, 6)    1       {b:2, c:1, d:1}', '"abra"    [2, 4)    1       {c:1}',
                 '""        [0, 12)   1       {a:5, b:2, c:1, d:1, r:2}', '"x"       empty     0       empty',
                 '"xcabra"  1         none     4   [2, 4)', '"xcabra"  2         none     4   [2, 4)',
                 '"xcabra"  3         none     1   [1, 6)   ("a")', '"xcabra"  1         2        2   [10, 12) ("ra")',
                 "SA = {11,10,7,0,3,5,8,1,4,6,9,2}", "sum(next) + at_end == hi - lo",
                 "lo + at_end + sum(next[b'] for b' < b)"):
        assert line in header, line
    _check_text(tb, oracle, np.random.default_rng(21))


def test_definitions_against_brute_force_golden(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        names = sorted(json.load(f))
    rng = np.random.default_rng(22)
    for name in names:
        with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
            _check_text(f.read(), oracle, rng)
    assert len(names) >= 5


@pytest.mark.parametrize("name", sorted(k for k, v in adversarial_cases().items() if len(v) <= 4097))
def test_definitions_against_brute_force_adversarial(oracle, name):
    tb = adversarial_cases()[name]
    _check_text(tb, oracle, np.random.default_rng(len(tb) + 2))


@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_definitions_against_brute_force_random(oracle, sigma):
    rng = np.random.default_rng(sigma)
    for n in (0, 1, 2, 7, 64, 65, 300, 1500):
        _check_text(rng.integers(0, sigma, n).astype(np.uint8).tobytes(), oracle, rng)


def test_route_models_and_their_bounds():
    """both routes give the counts of np.bincount on sorted runs of every shape; the streaming route probes cnt slots, the
    search route never more than 64 + 256 (ceil(log2(cnt + 1)) + 1)"""
    rng = np.random.default_rng(5)
    runs = [np.zeros(1), np.zeros(2), np.array([0, 255]), np.arange(256), np.repeat(np.arange(256), 2), np.repeat(np.arange(256), 301),
            np.r_[np.zeros(5000), np.arange(1, 256)], np.r_[np.arange(255), np.full(5000, 255)], np.full(70000, 7)]
    for cnt in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4096, 70001):
        for sigma in (1, 2, 4, 256):
            runs.append(np.sort(rng.integers(0, sigma, cnt)))
    for run in runs:
        want = np.bincount(run.astype(np.int64), minlength=256)
        got, probed = stream_route_model(run)
        assert np.array_equal(got, want) and probed == run.size
        got, probed = search_route_model(run)
        assert np.array_equal(got, want), run.size
        assert probed <= 64 + 255 * ceil_log2(run.size) <= search_route_bound(run.size), run.size
    assert search_route_model(np.repeat(np.arange(256), 301))[1] > 64 + 255       # (the bound is not vacuous: all 255 boundaries are searched)
    assert [route_of(c, 1024) for c in (0, 1, 1024, 1025)] == ["empty", "stream", "stream", "search"]
    assert [route_of(c, 0) for c in (0, 1)] == ["empty", "search"]


def test_backoff_model_and_its_bound():
    for cap in list(range(0, 70)) + [255, 256, 257, 4999, 5000, 2**31 - 1]:
        good, bad, probes = 0, cap + 1, 0
        while bad - good > 1:                                          # the bisection whatever the answers: always the lower half
            bad = (good + bad) // 2
            probes += 1
        good, bad, up = 0, cap + 1, 0
        while bad - good > 1:                                          # always the upper half
            good = (good + bad) // 2
            up += 1
        assert max(probes, up) == ceil_log2(cap + 1) <= backoff_bound(cap)
    assert (backoff_bound(0), backoff_bound(1), backoff_bound(256), backoff_bound(5000)) == (2, 4, 20, 28)


# ---------------------------------------------------------------- the surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    body = header[header.index("typedef struct sa_amd_ngram_stats"):header.index("} sa_amd_ngram_stats;")]
    declared = re.findall(r"^\s+int(64|32)_t\s+(\w+);", body, re.M)
    assert [name for _, name in declared] == list(STATS_FIELDS) == [name for name, _ in sa.NgramStats._fields_]
    for (bits, name), (_, ctype) in zip(declared, sa.NgramStats._fields_):
        assert ctypes.sizeof(ctype) * 8 == int(bits), name
    assert ctypes.sizeof(sa.NgramStats) == 9 * 8 + 4 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "ngram.hpp")) as f:
        kernels = f.read()
    m = re.search(r"constexpr int NG_STREAM_CAP_DEFAULT = ([^;]+);", kernels)
    assert m and int(m.group(1)) == sa.NGRAM_STREAM_CAP_DEFAULT == 1024


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.next_bytes) == ["self", "patterns", "dense"]
        assert params(cls.infgram) == ["self", "prompts", "min_count", "max_len"]
        assert inspect.signature(cls.next_bytes).parameters["dense"].default is False
        assert [inspect.signature(cls.infgram).parameters[k].default for k in ("min_count", "max_len")] == [1, 0]
    assert params(sa.ngram_set_stream_cap) == ["slots"] and params(sa.last_ngram_stats) == []
    for name in ("NgramStats", "last_ngram_stats", "ngram_set_stream_cap", "NGRAM_STREAM_CAP_DEFAULT"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert set(sa.last_ngram_stats()) == set(STATS_FIELDS)


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    g = good.ctypes.data
    assert L.sa_amd_index_next_bytes(None, p, g, 2, p, p, p, p, p, p, 4, c) == -1                # NULL index
    assert L.sa_amd_index_infgram(None, p, g, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(fake, p, g, -1, p, p, p, p, p, p, 4, c) == -1               # negative count, capacity
    assert L.sa_amd_index_next_bytes(fake, p, g, 2, p, p, p, p, p, p, -1, c) == -1
    assert L.sa_amd_index_infgram(fake, p, g, -1, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_infgram(fake, p, g, 2, 1, 0, p, p, p, p, p, p, p, -1, c) == -1
    for min_count in (0, -1, -2**31):                                                            # min_count < 1
        assert L.sa_amd_index_infgram(fake, p, g, 2, min_count, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_index_next_bytes(fake, p, None, 2, p, p, p, p, p, p, 4, c) == -1             # pat_off as sa_amd_index_search rejects it
    assert L.sa_amd_index_next_bytes(fake, None, g, 2, p, p, p, p, p, p, 4, c) == -1
    for off in bad:
        assert L.sa_amd_index_next_bytes(fake, p, off.ctypes.data, 2, p, p, p, p, p, p, 4, c) == -1
        assert L.sa_amd_index_infgram(fake, p, off.ctypes.data, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777)
    L.sa_amd_last_ngram_stats(None)


def test_stream_cap_switch():
    try:
        assert sa.ngram_set_stream_cap(100) == sa.NGRAM_STREAM_CAP_DEFAULT
        assert sa.ngram_set_stream_cap(0) == 100
        assert sa.ngram_set_stream_cap(2**40) == 0                     # a huge value is clamped, not refused
        assert sa.ngram_set_stream_cap(-1) == 2**31 - 1
        assert sa.ngram_set_stream_cap(-7) == 1024
    finally:
        sa.ngram_set_stream_cap(-1)
