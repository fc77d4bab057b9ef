"""CPU suite for matching a query against the index: the definitions of include/suffix_array_amd.h restated in numpy over the
oracle's suffix array, checked against literal brute force and against the identity that the cap of the shared spans costs
nothing; the oracle library's threaded restatement (the reference of the GPU suite at sizes the Python loop does not reach)
against the numpy one; the exports, the Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, adversarial_cases

EXPORTS = ("sa_amd_match_work_bytes", "sa_amd_index_match_stats", "sa_amd_index_match_stats_device", "sa_amd_index_match_spans",
           "sa_amd_index_match_spans_device", "sa_amd_last_match_stats", "sa_amd_match_set_group_cap", "sa_amd_match_set_group_lanes")
NONE = 0xFFFFFFFF
STAGE_MAX = 4096                                                      # what a workgroup of the group path stages at most


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def _lcp(x, y):
    k = min(len(x), len(y))
    if x[:k] == y[:k]:
        return k
    lo, hi = 0, k - 1                                                 # x[:lo] == y[:lo], x[:hi + 1] != y[:hi + 1]
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if x[:mid] == y[:mid]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def match_definition(t, arr, q, cap):
    """(ML, POS) as the header defines them: the lower bound of every window among the suffixes in slice order (bytes compare
    like Rust slices: lexicographic, a proper prefix is smaller), then its two neighbours"""
    tb, qb = t.tobytes(), q.tobytes()
    n, m = len(tb), len(qb)
    arr = np.asarray(arr, dtype=np.int64).tolist()
    ml = np.zeros(m, dtype=np.int64)
    pos = np.full(m, NONE, dtype=np.int64)
    for j in range(m):
        w = qb[j:j + cap]
        c = len(w)
        lo, hi = 0, n + 1
        while lo < hi:
            mid = (lo + hi) // 2
            p = arr[mid]
            if tb[p:p + c + 1] < w:                                   # (c + 1 bytes decide: a longer suffix that starts with w is not smaller)
                lo = mid + 1
            else:
                hi = mid
        i = lo
        assert 1 <= i <= n + 1
        a = _lcp(w, tb[arr[i - 1]:arr[i - 1] + c])
        b = _lcp(w, tb[arr[i]:arr[i] + c]) if i <= n else -1
        ml[j] = max(a, b)
        if ml[j] > 0:
            pos[j] = arr[i - 1] if a > b else arr[i]
    return ml, pos


def oracle_match_stats(oracle, t, arr, q, cap):
    """oracle_match_stats of oracle/oracle.c -> (ML, POS)"""
    L = oracle.L
    L.oracle_match_stats.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p]
    L.oracle_match_stats.restype = ctypes.c_int32
    t, q = np.ascontiguousarray(t, dtype=np.uint8), np.ascontiguousarray(q, dtype=np.uint8)
    a = np.ascontiguousarray(arr, dtype=np.uint32)
    assert a.size == t.size + 1
    out = np.full((2, q.size + 2), 0xEEEEEEEE, dtype=np.uint32)
    assert L.oracle_match_stats(t.ctypes.data, t.size, a.ctypes.data, q.ctypes.data, q.size, cap, out[0, 1:].ctypes.data,
                                out[1, 1:].ctypes.data) == 0
    assert np.all(out[:, 0] == 0xEEEEEEEE) and np.all(out[:, -1] == 0xEEEEEEEE)
    return out[0, 1:-1].astype(np.int64), out[1, 1:-1].astype(np.int64)


def union_spans(starts, lengths, m):
    """maximal intervals of the union of [s, s + len) -- ascending, disjoint, not adjacent -- as an (k, 2) array"""
    cover = np.zeros(m + 2, dtype=np.int64)
    for s, ln in zip(starts, lengths):
        cover[s] += 1
        cover[s + ln] -= 1
    on = np.cumsum(cover)[:m] > 0
    edge = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
    return np.stack([np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)], axis=1).astype(np.int64)


def spans_definition(t, arr, q, k):
    """-> (spans, flagged positions)"""
    ml, _ = match_definition(t, arr, q, k)
    flagged = np.flatnonzero(ml == k)
    return union_spans(flagged, [k] * flagged.size, q.size), flagged


def long_positions_definition(ml, m, cap, group_cap):
    """positions that leave the group path: the window is longer than the effective cap and some suffix agrees with it that far"""
    ge = min(group_cap, STAGE_MAX)
    c = np.minimum(cap, m - np.arange(m))
    return int(np.count_nonzero((c > ge) & (ml >= ge)))


def stats_definition(ml):
    best = int(ml.max()) if ml.size else 0
    return {"positions": int(ml.size), "matched": int(np.count_nonzero(ml)), "longest": best, "ml_sum": int(ml.sum()),
            "longest_pos": int(np.flatnonzero(ml == best)[0]) if best > 0 else -1}


def brute_ml(tb, qb, cap):
    """bytes.find on every window, binary search on the length"""
    out = []
    for j in range(len(qb)):
        lo, hi = 0, min(cap, len(qb) - j)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if tb.find(qb[j:j + mid]) >= 0:
                lo = mid
            else:
                hi = mid - 1
        out.append(lo)
    return np.array(out, dtype=np.int64)


def check_properties(t, q, ml, pos, cap):
    tb, qb = t.tobytes(), q.tobytes()
    m = len(qb)
    for j in range(m):
        if ml[j] == 0:
            assert pos[j] == NONE
        else:
            assert tb[int(pos[j]):int(pos[j]) + int(ml[j])] == qb[j:j + int(ml[j])], j
    assert np.all(ml <= np.minimum(cap, m - np.arange(m)))
    if cap >= m and m > 1:
        assert np.all(ml[1:] >= ml[:-1] - 1)


def _random_pair(rng):
    n, m = int(rng.integers(0, 60)), int(rng.integers(0, 60))
    sigma = int(rng.choice([1, 2, 3, 4, 26, 256]))
    return rng.integers(0, sigma, n).astype(np.uint8), rng.integers(0, sigma + int(rng.integers(0, 2)), m).astype(np.uint8)


def test_definition_against_brute_force(oracle):
    rng = np.random.default_rng(15)
    for trial in range(250):
        t, q = _random_pair(rng)
        arr = oracle.sais(t)
        for cap in (1, 2, 3, 7, int(rng.integers(1, 70)), q.size + 5):
            ml, pos = match_definition(t, arr, q, cap)
            assert np.array_equal(ml, brute_ml(t.tobytes(), q.tobytes(), cap)), (trial, cap)
            check_properties(t, q, ml, pos, cap)
    for name, b in adversarial_cases().items():
        t = _u8(b)
        if t.size > 600:
            continue
        arr = oracle.sais(t)
        for q in (t, t[1:], _u8(bytes(x ^ (i % 37 == 0) for i, x in enumerate(b)))):
            for cap in (1, 8, 65, t.size + 5):
                ml, pos = match_definition(t, arr, q, cap)
                assert np.array_equal(ml, brute_ml(t.tobytes(), q.tobytes(), cap)), (name, cap)
                check_properties(t, q, ml, pos, cap)


CAPS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 4096)                     # (tests/test_match.py runs the device over the same)


def queries(t, seed=0):
    """the query kinds of the GPU suite for one text"""
    tile = sa.MATCH_TILE
    rng = np.random.default_rng(seed)
    n = t.size
    changed = t.copy()
    changed[::37] ^= 1
    alphabet = np.unique(t) if n else np.array([65, 66], dtype=np.uint8)
    absent = np.setdiff1d(np.arange(256, dtype=np.uint8), np.unique(t))
    out = {"same": t, "changed": changed, "random": alphabet[rng.integers(0, alphabet.size, min(max(n, 5), 1500))],
           "empty": np.zeros(0, dtype=np.uint8)}
    if absent.size:
        out["absent"] = absent[rng.integers(0, absent.size, min(max(n, 3), 700))]
    for m in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
        out["m%d" % m] = np.resize(changed, m) if n else np.full(m, 65, dtype=np.uint8)
    return {k: np.ascontiguousarray(v, dtype=np.uint8) for k, v in out.items()}


def test_oracle_match_stats_equals_the_definition(oracle):
    texts = {name: _u8(b) for name, b in adversarial_cases().items() if len(b) <= 800}
    texts["english"] = corpus.english_corpus(3000, 8)
    texts["random2"] = np.random.default_rng(4).integers(0, 2, 2500, dtype=np.uint8)
    for name, t in texts.items():
        arr = oracle.sais(t)
        for qname, q in queries(t, 6).items():
            for cap in CAPS + (q.size + 5,):
                ml, pos = match_definition(t, arr, q, cap)
                got = oracle_match_stats(oracle, t, arr, q, cap)
                assert np.array_equal(got[0], ml) and np.array_equal(got[1], pos), (name, qname, cap)


def test_capped_union_equals_uncapped_union(oracle):
    rng = np.random.default_rng(16)
    for trial in range(200):
        t, q = _random_pair(rng)
        arr = oracle.sais(t)
        full, _ = match_definition(t, arr, q, q.size + 1)
        for k in (1, 2, 3, 5, int(rng.integers(1, 40))):
            spans, flagged = spans_definition(t, arr, q, k)
            keep = np.flatnonzero(full >= k)
            assert np.array_equal(spans, union_spans(keep, full[keep], q.size)), (trial, k)
            assert np.array_equal(flagged, keep)
            assert spans.shape[0] <= (q.size + 1) // (k + 1)
            if spans.size:
                assert np.all(spans[:, 1] - spans[:, 0] >= k) and np.all(spans[1:, 0] > spans[:-1, 1])


def test_known_answers(oracle):
    t, q = _u8(b"banana"), _u8(b"bandana")
    arr = oracle.sais(t)
    ml, pos = match_definition(t, arr, q, 8)
    assert ml.tolist() == [3, 2, 1, 0, 3, 2, 1] and pos.tolist() == [0, 1, 2, NONE, 3, 4, 5]
    ml, pos = match_definition(t, arr, q, 2)
    assert ml.tolist() == [2, 2, 1, 0, 2, 2, 1] and pos.tolist() == [0, 3, 2, NONE, 3, 4, 5]   # "an" is the lower bound itself: slot of "ana"
    assert spans_definition(t, arr, q, 2)[0].tolist() == [[0, 3], [4, 7]]
    assert spans_definition(t, arr, q, 3)[0].tolist() == [[0, 3], [4, 7]]
    assert spans_definition(t, arr, q, 4)[0].tolist() == []
    ml, pos = match_definition(_u8(b""), oracle.sais(b""), q, 4)
    assert not ml.any() and np.all(pos == NONE)
    ml, pos = match_definition(t, arr, _u8(b"xyz"), 4)
    assert not ml.any() and np.all(pos == NONE)
    assert stats_definition(match_definition(t, arr, q, 8)[0]) == {"positions": 7, "matched": 6, "longest": 3, "ml_sum": 12, "longest_pos": 0}
    assert long_positions_definition(np.array([3, 2, 1, 0, 3, 2, 1]), 7, 8, 2) == 3
    assert long_positions_definition(np.array([3, 2, 1, 0, 3, 2, 1]), 7, 8, 0) == 7
    assert long_positions_definition(np.array([3, 2, 1, 0, 3, 2, 1]), 7, 8, 64) == 0


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_MATCH_NONE\s+0xffffffffu\b", header)
    assert sa.MATCH_NONE == NONE
    body = header[header.index("typedef struct sa_amd_match_stats"):]
    for field in ("positions", "matched", "longest", "longest_pos", "ml_sum", "long_positions", "compared_bytes", "steps", "spans",
                  "covered_bytes", "flagged", "route_long", "readbacks", "group_lanes", "group_cap", "tile"):
        assert field in dict(sa.MatchStats._fields_), field
        assert re.search(r"\b" + field + r"\b", body), field
    assert ctypes.sizeof(sa.MatchStats) == 11 * 8 + 6 * 4


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(sa.DeviceIndex.match_stats) == ["self", "query", "max_len"]
    assert params(sa.DeviceIndex.match_spans) == ["self", "query", "min_len"]
    assert params(sa.SuffixArray.match_stats) == ["self", "query", "max_len"]
    assert params(sa.SuffixArray.match_spans) == ["self", "query", "min_len"]
    assert params(sa.match_stats_device_ptr) == ["index", "query_ptr", "m", "max_len", "ml_ptr", "pos_ptr", "work_ptr", "work_bytes", "stream"]
    assert params(sa.match_spans_device_ptr) == ["index", "query_ptr", "m", "min_len", "spans_ptr", "capacity", "work_ptr", "work_bytes",
                                                 "stream"]
    for name in ("MatchStats", "last_match_stats", "match_work_bytes", "match_set_group_cap", "match_set_group_lanes", "match_stats_device_ptr",
                 "match_spans_device_ptr", "MATCH_NONE", "MATCH_TILE"):
        assert name in sa.__all__ and hasattr(sa, name), name


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    cnt = ctypes.c_int64(-5)
    c = ctypes.byref(cnt)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    assert L.sa_amd_match_work_bytes(-1) == -1
    assert L.sa_amd_index_match_stats(None, p, 4, 4, p, p) == -1                               # NULL index
    assert L.sa_amd_index_match_stats_device(None, p, 4, 4, p, p, p, 1 << 20, None) == -1
    assert L.sa_amd_index_match_spans(None, p, 4, 4, p, 4, c) == -1
    assert L.sa_amd_index_match_spans_device(None, p, 4, 4, p, 4, c, p, 1 << 20, None) == -1
    assert L.sa_amd_index_match_stats(fake, p, -1, 4, p, p) == -1                              # m < 0
    assert L.sa_amd_index_match_stats(fake, None, 4, 4, p, p) == -1                            # NULL query
    assert L.sa_amd_index_match_stats(fake, p, 4, 0, p, p) == -1                               # max_len < 1
    assert L.sa_amd_index_match_stats_device(fake, p, 4, 0, p, p, p, 1 << 20, None) == -1
    assert L.sa_amd_index_match_stats_device(fake, None, 4, 4, p, p, p, 1 << 20, None) == -1
    assert L.sa_amd_index_match_spans(fake, p, 4, 0, p, 4, c) == -1                            # min_len < 1
    assert L.sa_amd_index_match_spans(fake, p, 4, 4, p, -1, c) == -1                           # negative capacity
    assert L.sa_amd_index_match_spans(fake, p, -1, 4, p, 4, c) == -1
    assert L.sa_amd_index_match_spans_device(fake, p, 4, 4, p, -1, c, p, 1 << 20, None) == -1
    assert L.sa_amd_index_match_spans_device(fake, p, 4, 0, p, 4, c, p, 1 << 20, None) == -1
    assert cnt.value == -5 and np.all(buf == 0x77777777)
    L.sa_amd_last_match_stats(None)


def test_group_cap_switch():
    try:
        assert sa.match_set_group_cap(8) == 64
        assert sa.match_set_group_cap(0) == 8
        assert sa.match_set_group_cap(1 << 30) == 0
        assert sa.match_set_group_cap(-1) == 1 << 20
        assert sa.match_set_group_cap(-7) == 64
        assert sa.match_set_group_lanes(4) == 8
        assert sa.match_set_group_lanes(100) == 4
        assert sa.match_set_group_lanes(9) == 16
        assert sa.match_set_group_lanes(-1) == 8
        assert sa.match_set_group_lanes(0) == 8
        assert sa.match_set_group_lanes(-1) == 4
    finally:
        sa.match_set_group_cap(-1)
        sa.match_set_group_lanes(-1)


@pytest.mark.parametrize("m", [0, 1, 255, 2048, 2049, 1 << 20, 2**31 - 1])
def test_work_block(m):
    """control words, a list entry and a flag byte per position, two words per span tile: about 5 m"""
    w = sa.match_work_bytes(m)
    assert w % 256 == 0 and 5 * m + 512 <= w <= 5 * m + 5 * 256 + 8 * (m // 2048 + 2) + 64
