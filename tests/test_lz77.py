"""GPU suite for the Lempel-Ziv factorisation: every route (host pointers with and without the array, device pointers,
DeviceIndex, SuffixArray) against the numpy definitions of test_lz77_abi.py over the oracle's suffix array; stage 1 alone on
permutations no short text produces; the walk's resume and restart routes; capacity, errors, the top of the size range; texts of
many phrases at every size where a stage changes, against the oracle library's linear-time factorisation."""
import ctypes
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, adversarial_cases
from test_lcp import _Dev, _u8, kasai
from test_lz77_abi import (LIT, _families, decode, lpf_definition, lpf_from_lcp, neighbour_slots, oracle_lz77, parse_definition,
                           stats_definition)

pytestmark = pytest.mark.gpu

N_ABOVE = (1 << 30) + 4097
CANARY = 0xA5
FAN, TILE = 32, 1024                                                  # stage 1: fan-out of the block minima, slots per tile
LCP_TILE = 2048
LENGTHS = (0, 1, 2, 3, TILE - 1, TILE + 1, LCP_TILE - 1, LCP_TILE + 1, 2 * LCP_TILE + 1, 8192, 8193, FAN ** 3, FAN ** 3 + 1)
_SAME = ("phrases", "literals", "longest", "longest_pos", "unresolved", "hierarchy_steps", "hierarchy_max", "walkers", "walk_steps",
         "walk_launches", "restarts", "splitter_spacing")


def levels(n):
    k = 2
    while -(-n // FAN ** k) > FAN:
        k += 1
    return k


def step_bound(n):
    """words one side of one slot may load (kernels/lz.hpp): 31 a level on the way up, 32 a level on the way down"""
    k = levels(n)
    return 31 * (k - 1) + 32 * k


def expected(oracle, t, arr=None):
    if arr is None:
        arr = oracle.sais(t)
    lpf, src = lpf_from_lcp(t, arr, kasai(oracle, t, arr))
    if t.size <= 600:
        lpf2, src2 = lpf_definition(t, arr)
        assert np.array_equal(lpf, lpf2) and np.array_equal(src, src2)
    return arr, lpf, src, parse_definition(lpf, src)


def lpf_on_device(t, arr, offset=0, want=(True, True)):
    """sa_amd_lpf_device on hipMalloc'ed buffers, `offset` bytes of misalignment in front of the text and 256 canary bytes on
    either side of both outputs"""
    n = t.size
    wb = sa.lz_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), 4 * n + 512, 4 * n + 512, wb) as d:
        dT, dS, dL, dR, dW = d.p
        for q in (dL, dR):
            assert d.hip.hipMemset(q, CANARY, 4 * n + 512) == 0
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        sa.lpf_device_ptr(dT + offset, dS, n, dL + 256 if want[0] else 0, dR + 256 if want[1] else 0, dW, wb)
        out = []
        for q, on in ((dL, want[0]), (dR, want[1])):
            raw = np.zeros(4 * n + 512, dtype=np.uint8)
            assert d.hip.hipMemcpy(raw.ctypes.data, q, raw.size, 2) == 0
            assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 4 * n:] == CANARY)
            if not on:
                assert np.all(raw == CANARY)
            out.append(raw[256:256 + 4 * n].view(np.uint32).astype(np.int64))
    return out


def parse_on_device(t, arr, capacity, offset=0):
    """sa_amd_lz77_device likewise; returns (count, the phrases that came back)"""
    n = t.size
    wb = sa.lz_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), 8 * capacity + 512, wb) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * capacity + 512) == 0
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        count = sa.lz77_device_ptr(dT + offset, dS, n, dO + 256, capacity, dW, wb)
        raw = np.zeros(8 * capacity + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
    assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 8 * capacity:] == CANARY)
    body = raw[256:256 + 8 * capacity]
    wrote = min(count, capacity)
    assert np.all(body[8 * wrote:] == CANARY)                         # nothing behind the phrases that exist
    return count, body[:8 * wrote].view(np.uint32).reshape(-1, 2).astype(np.int64)


def check_stats(ph, n, got=None):
    got = sa.last_lz_stats() if got is None else got
    for key, val in stats_definition(ph).items():
        assert got[key] == val, (key, got)
    assert got["readbacks"] >= 1 and got["hierarchy_max"] <= step_bound(max(n, 1))
    return {k: got[k] for k in _SAME}


def check_all_routes(oracle, t, name="", offsets=(0,), arr=None):
    n = t.size
    arr, lpf, src, ph = expected(oracle, t, arr)

    def same(got, exp):
        return got.dtype == np.uint32 and got.shape == exp.shape and np.array_equal(got, exp)
    g = sa.lpf(t)
    assert same(g[0], lpf) and same(g[1], src), name
    st = sa.last_lz_stats()
    assert st["phrases"] == 0 and st["longest_pos"] == -1 and st["splitter_spacing"] == 0
    g = sa.lpf(t, arr)
    assert same(g[0], lpf) and same(g[1], src), name
    got = sa.lz77(t)
    assert same(got, ph), name
    assert decode(got, t) == t.tobytes(), name
    first = check_stats(ph, n)
    assert same(sa.lz77(t, arr), ph), name
    assert check_stats(ph, n) == first, name
    ix = sa.DeviceIndex(t, arr)
    s = sa.SuffixArray.unchecked_from_parts(t, arr)
    g = ix.lpf()
    assert same(g[0], lpf) and same(g[1], src), name
    assert same(ix.lz77(), ph), name
    assert check_stats(ph, n) == first, name
    g = s.lpf()
    assert same(g[0], lpf) and same(g[1], src), name
    assert same(s.lz77(), ph), name
    ix.close()
    for off in offsets:
        a, b = lpf_on_device(t, arr, off)
        assert np.array_equal(a, lpf) and np.array_equal(b, src), (name, off)
        count, dev = parse_on_device(t, arr, max(n, 1), off)
        assert count == ph.shape[0] and np.array_equal(dev, ph), (name, off)
        assert check_stats(ph, n) == first, (name, off)
    return ph


def test_known_answers():
    t = _u8(b"banana")
    lpf, src = sa.lpf(t)
    assert lpf.tolist() == [0, 0, 0, 3, 2, 1] and src.tolist() == [LIT, LIT, LIT, 1, 2, 3]
    assert sa.lz77(t).tolist() == [[LIT, 1], [LIT, 1], [LIT, 1], [1, 3]]
    st = sa.last_lz_stats()
    assert (st["phrases"], st["literals"], st["longest"], st["longest_pos"]) == (4, 3, 3, 3)
    assert sa.lz77(b"").shape == (0, 2) and sa.last_lz_stats()["longest_pos"] == -1
    g = sa.lpf(b"")
    assert g[0].shape == (0,) and g[1].shape == (0,)
    assert sa.lz77(b"x").tolist() == [[LIT, 1]]
    assert sa.lz77(b"a" * 50).tolist() == [[LIT, 1], [0, 49]]
    assert sa.lz77(b"ab" * 20).tolist() == [[LIT, 1], [LIT, 1], [0, 38]]


def test_tiny_texts_all_routes(oracle):
    for b in (b"", b"a", b"aa", b"ab", b"ba", b"aba", b"abc"):
        check_all_routes(oracle, _u8(b), b, offsets=(0, 1, 2, 3))


def test_adversarial_cases_all_routes(oracle):
    for name, b in adversarial_cases().items():
        t = _u8(b)
        check_all_routes(oracle, t, name, offsets=(0, 1, 2, 3) if t.size <= 600 else (3,))


def test_golden_fixtures(oracle):
    import json
    import os
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "manifest.json")) as f:
        names = sorted(json.load(f))
    assert names
    for name in names:
        t = np.fromfile(os.path.join(gold, name + ".text"), dtype=np.uint8)
        arr = np.fromfile(os.path.join(gold, name + ".sa.u32le"), dtype="<u4")
        check_all_routes(oracle, t, name, arr=arr)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_where_a_stage_changes(oracle, n):
    check_all_routes(oracle, corpus.english_corpus(n, 5) if n else _u8(b""), n, offsets=(0, 1))
    check_all_routes(oracle, np.random.default_rng(n).integers(0, 2, n, dtype=np.uint8), n)
    check_all_routes(oracle, np.full(n, 7, dtype=np.uint8), n)


@pytest.mark.parametrize("family", sorted(_families(8)))
def test_text_families(oracle, family):
    for n in (3001, 20000):
        check_all_routes(oracle, _families(n)[family], (family, n), offsets=(2,))


def test_all_distinct_bytes(oracle):
    check_all_routes(oracle, np.arange(256, dtype=np.uint8), "ascending", offsets=(0, 1))
    check_all_routes(oracle, np.arange(255, -1, -1, dtype=np.uint8), "descending", offsets=(0, 1))


@pytest.mark.parametrize("cap", [0, 1, 64, 1 << 20])
def test_compare_cap_routes(oracle, cap):
    """the value stage's short and long compare paths, on either side of the per-lane cap"""
    prev = sa.lcp_set_compare_cap(cap)
    try:
        for name in ("twice", "fibonacci", "random4", "one_byte"):
            t = _families(5000)[name]
            check_all_routes(oracle, t, (name, cap))
            if name in ("twice", "one_byte"):
                assert (sa.last_lcp_stats()["long_pairs"] > 0) == (cap < 1 << 20), (name, cap)
    finally:
        sa.lcp_set_compare_cap(prev)


# ---------------------------------------------------------------- stage 1 alone ----

def _permutations(m):
    rng = np.random.default_rng(m)
    up = np.arange(m, dtype=np.uint32)
    out = {"ascending": up, "descending": up[::-1].copy(), "random": rng.permutation(m).astype(np.uint32),
           "organ_pipe": np.concatenate([up[0::2], up[1::2][::-1]])}
    if m > 2 * TILE:                                                  # whole tiles ascending, the smallest values in the last tile:
        saw = up.copy()                                               # every slot in front of it finds its right answer there
        saw[:m - TILE] += TILE
        saw[m - TILE:] -= m - TILE
        out["sawtooth_right"] = saw
        out["sawtooth_left"] = saw[::-1].copy()
        teeth = (up % TILE) * ((m + TILE - 1) // TILE) + (up // TILE)  # teeth one tile long, every tooth above the one in front
        out["teeth"] = teeth.astype(np.uint32)
        out["teeth_down"] = teeth[::-1].astype(np.uint32).copy()
    return out


def nsv_on_device(a):
    L = sa.diag_lib()
    m = a.size
    counters = (ctypes.c_int64 * 4)()
    with _Dev(4 * m, 4 * m + 512, 4 * m + 512) as d:
        dA, dP, dN = d.p
        assert d.hip.hipMemcpy(dA, a.ctypes.data, 4 * m, 1) == 0
        for q in (dP, dN):
            assert d.hip.hipMemset(q, CANARY, 4 * m + 512) == 0
        assert L.sa_amd_test_lz_nsv(dA, m, dP + 256, dN + 256, counters) == 0
        out = []
        for q in (dP, dN):
            raw = np.zeros(4 * m + 512, dtype=np.uint8)
            assert d.hip.hipMemcpy(raw.ctypes.data, q, raw.size, 2) == 0
            assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 4 * m:] == CANARY)
            out.append(raw[256:256 + 4 * m].view(np.int32).astype(np.int64))          # (0xffffffff reads as -1)
    return out[0], out[1], list(counters)


@pytest.mark.parametrize("m", [1, 2, 3, TILE - 1, TILE, TILE + 1, LCP_TILE + 1, 8193, FAN ** 3, FAN ** 3 + 1, 100003, FAN ** 4, FAN ** 4 + 1])
def test_nearest_smaller_values(m):
    for name, a in _permutations(m).items():
        if m > 200000 and name not in ("random", "sawtooth_right", "teeth_down", "descending"):
            continue
        psv, nsv = neighbour_slots(a)
        gp, gn, counters = nsv_on_device(np.ascontiguousarray(a, dtype=np.uint32))
        assert np.array_equal(gp, psv) and np.array_equal(gn, nsv), (name, m)
        assert counters[3] == levels(m) and counters[2] <= step_bound(m), (name, m, counters)
        assert counters[1] <= 2 * m * step_bound(m)
        if name == "sawtooth_right":
            assert counters[0] >= m - TILE                            # every slot in front of the last tile leaves its tile
        print(name, m, "unresolved", counters[0], "steps", counters[1], "max", counters[2], "levels", counters[3])


def test_values_that_are_no_positions():
    """the diagnostic entry takes any distinct values: the top of the uint32 range included"""
    a = (np.random.default_rng(5).permutation(5000).astype(np.uint32) * np.uint32(858993) + np.uint32(123456789))
    a[17] = 0xFFFFFFFF
    assert np.unique(a).size == a.size
    psv, nsv = neighbour_slots(a)
    gp, gn, _ = nsv_on_device(a)
    assert np.array_equal(gp, psv) and np.array_equal(gn, nsv)


# ---------------------------------------------------------------- the walk ----

def test_walk_resume_and_restart_routes(oracle):
    t = corpus.english_corpus(6000, 9)
    arr, lpf, src, ph = expected(oracle, t)
    assert np.array_equal(sa.lz77(t, arr), ph)
    base = sa.last_lz_stats()
    assert base["restarts"] == 0 and base["splitter_spacing"] == 256
    try:
        sa.unbwt_set_walk_limits(1, 2)                                # one step a launch, two launches an attempt
        assert np.array_equal(sa.lz77(t, arr), ph)
        st = check_stats(ph, t.size)
        assert st["restarts"] >= 1 and st["splitter_spacing"] == 4 and st["walk_launches"] > 2 * (st["restarts"] + 1)
        sa.unbwt_set_walk_limits(7, -1)                               # resumed walks, no restart
        assert np.array_equal(sa.lz77(t, arr), ph)
        st = check_stats(ph, t.size)
        assert st["restarts"] == 0 and st["walk_launches"] > 1
        sa.unbwt_set_walk_limits(-1, -1)
        for spacing in (4, 65536):
            sa.unbwt_set_splitter_spacing(spacing)
            assert np.array_equal(sa.lz77(t, arr), ph), spacing
            st = check_stats(ph, t.size)
            assert st["splitter_spacing"] == spacing and st["restarts"] == 0
            assert st["walkers"] >= (t.size // 16 if spacing == 4 else 1)
        t2 = np.random.default_rng(8).integers(0, 256, 30000, dtype=np.uint8)      # thousands of phrases behind one sparse splitter
        _, _, _, ph2 = expected(oracle, t2)
        sa.unbwt_set_walk_limits(1000, -1)
        assert np.array_equal(sa.lz77(t2), ph2)
        assert sa.last_lz_stats()["walk_launches"] >= 2
    finally:
        sa.unbwt_set_walk_limits(-1, -1)
        sa.unbwt_set_splitter_spacing(-1)
    assert np.array_equal(sa.lz77(t, arr), ph)
    assert {k: v for k, v in sa.last_lz_stats().items() if k != "readbacks"} == {k: v for k, v in base.items() if k != "readbacks"}


# ---------------------------------------------------------------- capacity, errors ----

def test_capacity(oracle):
    t = corpus.english_corpus(50000, 12)
    arr, lpf, src, ph = expected(oracle, t)
    z = ph.shape[0]
    assert z > 8
    for cap in (0, 1, z - 1, z, z + 1):
        count, dev = parse_on_device(t, arr, cap)
        assert count == z and np.array_equal(dev, ph[:cap]), cap
        check_stats(ph, t.size)
    out = np.full((5, 2), 0xEEEEEEEE, dtype=np.uint32)
    cnt = ctypes.c_int64(0)
    assert sa.lib().sa_amd_lz77(t.ctypes.data, t.size, None, out.ctypes.data, 3, ctypes.byref(cnt)) == 0
    assert cnt.value == z and np.array_equal(out[:3], ph[:3]) and np.all(out[3:] == 0xEEEEEEEE)
    check_stats(ph, t.size)
    a, b = lpf_on_device(t, arr, 1, want=(True, False))
    assert np.array_equal(a, lpf)
    a, b = lpf_on_device(t, arr, 1, want=(False, True))
    assert np.array_equal(b, src)


def test_errors():
    L = sa.lib()
    t = _u8(b"mississippi")
    n = t.size
    arr = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, arr)
    out = np.full(2 * n + 2, 0x77777777, dtype=np.uint32)
    cnt = ctypes.c_int64(-5)
    c = ctypes.byref(cnt)
    bad = arr.copy()
    bad[5] = n + 1
    assert L.sa_amd_lpf(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, out.ctypes.data) == -6
    assert L.sa_amd_lz77(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, n, c) == -6
    with pytest.raises(IndexError):
        sa.lpf(t, bad)
    with pytest.raises(IndexError):
        sa.lz77(t, bad)
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]
    assert L.sa_amd_lpf(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert L.sa_amd_lz77(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, n, c) == -1
    with pytest.raises(ValueError):
        sa.lz77(t, bad)
    assert L.sa_amd_lz77(t.ctypes.data, n, arr.ctypes.data, out.ctypes.data, -1, c) == -1                   # negative capacity
    assert cnt.value == -5 and np.all(out == 0x77777777)                                                     # nothing written
    assert L.sa_amd_lz77(None, 0, np.array([1], dtype=np.uint32).ctypes.data, None, 0, c) == -6
    assert L.sa_amd_lz77(None, 0, np.array([0], dtype=np.uint32).ctypes.data, None, 0, c) == 0 and cnt.value == 0
    wb = sa.lz_work_bytes(n)
    with _Dev(n, 4 * (n + 1), 8 * n + 512, wb + 256) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * n + 512) == 0
        assert d.hip.hipMemcpy(dS, arr.ctypes.data, 4 * (n + 1), 1) == 0
        assert d.hip.hipMemcpy(dT, t.ctypes.data, n, 1) == 0
        cnt.value = -5
        assert L.sa_amd_lpf_device(dT, dS, n, dO, dO + 4 * n, dW, 64, None) == -1                           # short work block
        assert L.sa_amd_lpf_device(dT, dS, n, dO, dO + 4 * n, dW + 4, wb, None) == -1                       # misaligned work block
        assert L.sa_amd_lz77_device(dT, dS, n, dO, n, c, dW + 128, wb, None) == -1
        assert L.sa_amd_lz77_device(dT, dS, n, dO, n, c, dW, wb - 256, None) == -1
        assert L.sa_amd_lz77_device(dT, dS, n, dO, -1, c, dW, wb, None) == -1
        raw = np.zeros(8 * n + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
        assert np.all(raw == CANARY) and cnt.value == -5
        assert L.sa_amd_lz77_device(dT, dS, n, dO, n, c, dW, wb, None) == 0 and cnt.value == sa.lz77(t).shape[0]


def test_wrong_permutation_terminates_in_bounds():
    """duplicate entries: unspecified answers, but the outputs' canaries hold, the lengths stay inside the text and the call ends"""
    rng = np.random.default_rng(77)
    n = 50000
    t = corpus.english_corpus(n, 2)
    arr = np.empty(n + 1, dtype=np.uint32)
    arr[0] = n
    arr[1:] = rng.integers(0, n, n)                                   # in range, SA[0] = n, far from a permutation
    lpf_on_device(t, arr, 1)
    count, dev = parse_on_device(t, arr, n)
    assert 0 < count <= n and np.all(dev[:, 1] >= 1)
    good = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, good)
    good[100], good[200] = good[200], good[100]                       # a permutation, not the suffix array
    lpf_on_device(t, good, 0)
    count, dev = parse_on_device(t, good, n)
    assert 0 < count <= n


# ---------------------------------------------------------------- many phrases at the sizes where a stage changes ----
# The minima hierarchy gains a level above FAN^3 and above FAN^4 slots; k_unbwt_splitters strides once its grid is capped at
# 16 384 workgroups of 256 lanes and k_lz_merge once its grid is capped at 65 536 (host/lz.hpp).  The reference is oracle_lz77
# (oracle/oracle.c) over oracle.sais: the numpy definitions do not reach these sizes.
SPLITTER_GRID_SPAN = 16384 * 256
MERGE_GRID_SPAN = 65536 * 256
MID_SIZES = (FAN ** 3, FAN ** 3 + 1, 2 * FAN ** 3 + 1, FAN ** 4, FAN ** 4 + 1)
LARGE_SIZES = (SPLITTER_GRID_SPAN + 257, MERGE_GRID_SPAN + 1025)
DEVICE_FORMS_UP_TO = 2 * FAN ** 3 + 1
SHARED = ("english", FAN ** 4 + 1)                                    # the text of the capacity and the walk test
_REFERENCE = {}


def _big_text(family, n):
    if family == "english":
        return corpus.english_corpus(n, 17)
    if family == "dna_repeats":
        return corpus.dna_repeats(n, 18)
    rng = np.random.default_rng(n)
    if family == "random2":
        return rng.integers(0, 2, n, dtype=np.uint8)
    assert family == "twice"
    h = rng.integers(0, 256, n // 2, dtype=np.uint8)
    return np.ascontiguousarray(np.resize(np.concatenate([h, h]), n))


def big_reference(oracle, family, n):
    """(text, array, LPF, SRC, phrases) by oracle.sais and oracle_lz77, computed once and left unchanged"""
    if (family, n) in _REFERENCE:
        return _REFERENCE[family, n]
    t = _big_text(family, n)
    arr = oracle.sais(t)
    lpf, src, ph, z = oracle_lz77(oracle, t, arr)
    assert z == ph.shape[0]
    for a in (t, arr, lpf, src, ph):
        a.flags.writeable = False
    if (family, n) == SHARED:
        _REFERENCE[family, n] = (t, arr, lpf, src, ph)
    return t, arr, lpf, src, ph


def check_big_text(oracle, family, n):
    t, arr, lpf, src, ph = big_reference(oracle, family, n)
    top = levels(n)
    assert top == (2 if n <= FAN ** 3 else 3 if n <= FAN ** 4 else 4 if n <= FAN ** 5 else 5)
    g = sa.lpf(t, arr)
    st = sa.last_lz_stats()
    assert g[0].dtype == np.uint32 and g[1].dtype == np.uint32
    assert np.array_equal(g[0], lpf), (family, n, np.flatnonzero(g[0] != lpf)[:8])
    assert np.array_equal(g[1], src), (family, n, np.flatnonzero(g[1] != src)[:8])
    assert st["hierarchy_max"] <= step_bound(n) and st["phrases"] == 0
    del g
    got = sa.lz77(t, arr)
    assert got.shape == ph.shape, (family, n, got.shape, ph.shape)
    assert np.array_equal(got, ph), (family, n, np.flatnonzero((got != ph).any(axis=1))[:8])
    st = check_stats(ph, n)
    assert st["hierarchy_max"] <= step_bound(n)
    assert decode(got, t) == t.tobytes(), (family, n)
    print(family, n, "levels", top, "phrases", ph.shape[0], {k: st[k] for k in ("unresolved", "hierarchy_max", "walkers", "walk_launches")})
    if n <= DEVICE_FORMS_UP_TO:
        a, b = lpf_on_device(t, arr, 1)
        assert np.array_equal(a, lpf) and np.array_equal(b, src), (family, n)
        count, dev = parse_on_device(t, arr, n, 3)
        assert count == ph.shape[0] and np.array_equal(dev, ph), (family, n)
        assert check_stats(ph, n) == st, (family, n)
    return ph


def test_stage_thresholds_follow_the_constants():
    """the sizes above are the first at which the code takes the other path"""
    assert (levels(FAN ** 3), levels(FAN ** 3 + 1), levels(FAN ** 4), levels(FAN ** 4 + 1)) == (2, 3, 3, 4)
    assert FAN * FAN == TILE and sa.MATCH_TILE == 256
    for n, span in zip(LARGE_SIZES, (SPLITTER_GRID_SPAN, MERGE_GRID_SPAN)):
        assert -(-n // 256) > span // 256                              # more workgroups' worth of slots than the capped grid


@pytest.mark.parametrize("n", MID_SIZES)
@pytest.mark.parametrize("family", ["english", "dna_repeats", "random2", "twice"])
def test_many_phrases_where_the_hierarchy_gains_a_level(oracle, family, n):
    """a real suffix array under three and four levels of minima, k_lz_far<true> through them, thousands of walkers through the
    doubling rounds, phrase counts summed over hundreds of emit tiles.  (oracle.sais + oracle_lz77 at 1 048 577 bytes: 0.13 s on
    one host core.)"""
    ph = check_big_text(oracle, family, n)
    assert ph.shape[0] > n // 64                                      # many phrases: every emit tile holds some


@pytest.mark.parametrize("n", LARGE_SIZES)
@pytest.mark.parametrize("family", ["english", "random2"])
def test_many_phrases_where_a_capped_grid_strides(oracle, family, n):
    """k_unbwt_splitters above 16 384 workgroups' worth of positions, k_lz_merge above 65 536.  (The CPU reference takes longer
    than the device: oracle.sais + oracle_lz77 at 16 778 241 bytes took 2.3 s + 1.4 s on one host core.)"""
    ph = check_big_text(oracle, family, n)
    assert ph.shape[0] > n // 64


def test_cut_capacity_at_four_levels(oracle):
    """fewer places than phrases at 1 048 577 bytes: the true count, the true prefix, nothing behind it"""
    t, arr, lpf, src, ph = big_reference(oracle, *SHARED)
    z = ph.shape[0]
    assert z > 4096
    for cap in (z - 1, z, z // 2):
        count, dev = parse_on_device(t, arr, cap, 1)                  # (checks the canaries on either side and behind the phrases)
        assert count == z and np.array_equal(dev, ph[:cap]), cap
        check_stats(ph, t.size)


def test_walk_resumes_at_four_levels(oracle):
    """64 steps a launch: k_lz_walk and k_lz_flag go on where the launch before stopped, over thousands of walkers"""
    t, arr, lpf, src, ph = big_reference(oracle, *SHARED)
    try:
        sa.unbwt_set_walk_limits(64, -1)
        got = sa.lz77(t, arr)
        assert np.array_equal(got, ph)
        st = check_stats(ph, t.size)
        assert st["restarts"] == 0 and st["walk_launches"] > 1 and st["splitter_spacing"] == 256
        assert st["walkers"] > t.size // 1024
        sa.unbwt_set_walk_limits(16, 3)                               # three launches an attempt: denser splitters, another seed
        assert np.array_equal(sa.lz77(t, arr), ph)
        st = check_stats(ph, t.size)
        assert st["restarts"] >= 1 and st["splitter_spacing"] < 256
    finally:
        sa.unbwt_set_walk_limits(-1, -1)
    assert np.array_equal(sa.lz77(t, arr), ph)
    st = sa.last_lz_stats()
    assert st["restarts"] == 0 and st["splitter_spacing"] == 256      # the defaults are back


# ---------------------------------------------------------------- the top of the size range ----

def _period2_array(n):
    """suffix array of (1 2)^k 1, n odd: the suffixes that start with 1, shortest first, then those that start with 2"""
    assert n % 2 == 1
    arr = np.empty(n + 1, dtype=np.uint32)
    arr[0] = n
    h = (n + 1) // 2
    arr[1:1 + h] = np.arange(n - 1, -1, -2, dtype=np.uint32)
    arr[1 + h:] = np.arange(n - 2, 0, -2, dtype=np.uint32)
    return arr


def test_period2_array_is_the_suffix_array(oracle):
    for n in (1, 3, 5, 99):
        t = np.resize(np.array([1, 2], dtype=np.uint8), n)
        assert np.array_equal(_period2_array(n), oracle.sais(t))


@pytest.mark.parametrize("family", ["one_byte", "period2"])
def test_above_1gib_closed_form(family):
    n = N_ABOVE
    if family == "one_byte":
        t = np.full(n, 0x41, dtype=np.uint8)
        arr = np.arange(n, -1, -1, dtype=np.uint32)
        exp = [[LIT, 1], [0, n - 1]]
    else:
        t = np.resize(np.array([1, 2], dtype=np.uint8), n)
        arr = _period2_array(n)
        exp = [[LIT, 1], [LIT, 1], [0, n - 2]]
    ix = sa.DeviceIndex(t, arr)
    del arr
    got = ix.lz77()
    st = sa.last_lz_stats()
    assert got.tolist() == exp
    assert st["phrases"] == len(exp) and st["literals"] == len(exp) - 1 and st["longest"] == exp[-1][1] and st["longest_pos"] == len(exp) - 1
    assert st["hierarchy_max"] <= step_bound(n)
    ix.close()
    print(family, st, sa.last_lcp_stats())
    del t
    sa.lib().sa_amd_release_cache()


def test_thread_safety(oracle):
    texts = [corpus.english_corpus(60000 + 1000 * j, 20 + j) for j in range(4)]
    exp = [expected(oracle, t) for t in texts]
    errors = []

    def work(j):
        try:
            for _ in range(3):
                got = sa.lz77(texts[j])
                st = sa.last_lz_stats()
                assert np.array_equal(got, exp[j][3])
                check_stats(exp[j][3], texts[j].size, st)
                g = sa.lpf(texts[j])
                assert np.array_equal(g[0], exp[j][1]) and np.array_equal(g[1], exp[j][2])
                assert sa.last_lz_stats()["phrases"] == 0
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
