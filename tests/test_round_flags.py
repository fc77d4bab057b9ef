"""Status bytes of the dense doubling rounds: k_group_sort<..., STATUS> (kernels/refine.hpp) writes one byte per list member and no
key for the members it orders, and the round's re-rank (rr_wave_classify_status, kernels/rerank.hpp) reads the group starts
from the bytes, taking keys only where a member was left to another kernel.

The product library has no switch: it takes the byte route wherever a dead device slab exists for the bytes.  The diagnostic
library, built from the same sources, takes the mode from sa_amd_debug_round_flags: 0 = never (the key route, what the parent
commit did), 1 = the rule, 2 = the rule with the round's key buffer and status slab poisoned before the local pass.  Every build
below runs in the diagnostic library under modes 0, 1 and 2 and in the product library; in each of them the array is the
oracle's, and the statistics and the per-round tied counts of the trace are those of mode 0.

The texts are the smallest shapes at which the rule can go wrong: the boundaries are the k_group_sort tile (2 048 members), the
re-rank wave (512) and the re-rank tile (8 192).  (A tied list of ONE member does not exist -- a member is tied with a neighbour --
so the list lengths start at 2.)"""
import ctypes
import functools
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word
import refinement_model as rm

KEY_SYMBOLS = 8          # random bytes: 8-bit symbols, 8 to a 64-bit key (the list-length texts below count on it and assert it)

REGIMES = [
    {"SA_AMD_FORCE_DENSE": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_BINNED_ISA": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_CHASE": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_CHASE": "3"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_CHASE": "7"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_DEFER": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_BIG_GROUP_SORT": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_GROUP_CAP": "64"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NETWORK_MIN": "0"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NETWORK_MIN": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_FIRST_TAIL": "1"},
    {"SA_AMD_NO_TEXT_ROUNDS": "1"},
]
_IDS = lambda r: ",".join(f"{k[7:]}={v}" for k, v in r.items())      # noqa: E731

BY_STATUS, BY_KEYS = "(group starts read from status bytes)", "(group starts read from keys)"
_MISSES = re.compile(r"\((\d+) rounds deferred their mid-round count and had to run the global sort after all\)")


def _rnd(seed, count, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, count, dtype=np.uint8)


def _list_length_text(m):
    """a text whose tied list behind the initial sort has exactly m members: random bytes, with one block of m // 2 + 7 bytes
    copied twice (a pair of tied suffixes for every offset that leaves KEY_SYMBOLS bytes of the block) and, for an odd m, one
    block of 8 bytes copied three times"""
    pairs = (m - 3) // 2 if m % 2 else m // 2
    B, C = _rnd(7000 + m, pairs + KEY_SYMBOLS - 1), _rnd(8000 + m, KEY_SYMBOLS)
    parts = [_rnd(9000 + m, 3000), B, _rnd(9001 + m, 1500), B, _rnd(9002 + m, 2500)]
    if m % 2:
        parts += [C, _rnd(9003 + m, 700), C, _rnd(9004 + m, 900), C, _rnd(9005 + m, 1100)]
    return np.concatenate(parts)


def _keyed_between_owned(copies, pairs_shift):
    """Groups no tile of k_group_sort can own, directly behind and directly in front of groups that tiles do own, with their
    first members on re-rank wave and tile starts.  In the order of the list:
      1. 4 096 pairs (two copies of a block over the byte values below 0x10): 8 192 owned members, one re-rank tile -- when the
         key holds pairs_shift + 1 symbols; the callers sweep pairs_shift, so that one text of the family has exactly 8 192;
      2. a block of 24 bytes repeated `copies` times (a multiple of 512): one group of exactly `copies` members for each of
         its first 8 offsets -- the last 16 bytes of the block are its largest, so the groups of the offsets whose last copy
         runs into the end of the repeats (and has fewer members) come behind these --, every first member on a wave start
         and, every 8 192 members, on a tile start;
      3. text with many small groups (English-like, moved above the block's byte values): owned members, and enough of them
         that the members of 2. are less than half of the text (they go through the gather and the scatter, not the
         whole-list sort)."""
    small = _rnd(100 + pairs_shift, 4096 + pairs_shift, 0, 0x10)
    block = np.concatenate([_rnd(200 + copies, 8, 0x10, 0x60), np.arange(0x60, 0x70, dtype=np.uint8)])
    english = (corpus.english(max(60_000, 25 * copies), 21) + np.uint8(0x60)).astype(np.uint8)
    tail = np.arange(0xF0, 0x100, dtype=np.uint8)
    return np.concatenate([small, small, np.tile(block, copies), tail, english])


@functools.lru_cache(maxsize=None)
def _texts():
    out = [(name, np.frombuffer(b, dtype=np.uint8).copy()) for name, b in adversarial_cases().items()]
    out.append(("fibonacci", np.frombuffer(fibonacci_word(24)[:100_000], dtype=np.uint8).copy()))
    for n in (8193, 65537, (1 << 20) + 3):
        out.append((f"english_{n}", corpus.english(n, 5)))
    block = corpus.english(8192, 11)
    out.append(("period_8192", np.concatenate([block] * 5 + [block[:7]])))       # equal keys on every tile seam
    out.append(("one_byte_value", np.full(20000, 0x61, dtype=np.uint8)))           # (the suite runs with the unary shortcut off: the whole list through the global sort behind a local pass)
    # groups of 97, 700 and 1 024 members: counting, the network, the straddle kernel
    for period, copies in ((700, 97), (333, 700), (211, 1024)):
        rng = np.random.default_rng(period * 7 + copies)
        blk = rng.integers(0, 256, period, dtype=np.uint8)
        out.append((f"blocks_{period}x{copies}", np.tile(blk, copies)))
        out.append((f"blocks_{period}x{copies}_mixed", np.concatenate([np.tile(blk, copies // 2), corpus.english(50_000, 3), np.tile(blk[: period // 3], copies),
                                                                       rng.integers(0, 3, 20_000, dtype=np.uint8)])))
    # groups of 2 048 and 8 192 members (k_group_sort_big, both instances) and of 16 384 (the global sort), see _keyed_between_owned
    for copies in (2048, 8192, 16384):
        for shift in (KEY_SYMBOLS - 2, KEY_SYMBOLS - 1, KEY_SYMBOLS):
            out.append((f"keyed_{copies}_{shift}", _keyed_between_owned(copies, shift)))
    for m in (2, 2047, 2048, 2049, 8191, 8192, 8193):
        out.append((f"list_of_{m}", _list_length_text(m)))
    return tuple(out)


_expected = {}


def _oracle_sa(oracle, name, t):
    if name not in _expected:
        _expected[name] = oracle.sais(t)
    return _expected[name]


def _build(monkeypatch, capfd, env, t, mode):
    """(array, statistics, stderr) of one traced host-pointer build: mode None = the product library, else the diagnostic library
    in that mode"""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        m.setenv("SA_AMD_VERBOSE", "3")
        capfd.readouterr()
        if mode is None:
            out, st = sa.SuffixArray(t).into_parts()[1], sa.last_stats()
        else:
            L = sa.diag_lib()
            t = np.ascontiguousarray(t)
            out = np.zeros(t.size + 1, dtype=np.uint32)
            stats = sa.Stats()
            before = L.sa_amd_debug_round_flags(mode)
            try:
                assert L.sa_amd_saca_u8(t.ctypes.data if t.size else None, out.ctypes.data, t.size) == 0
            finally:
                L.sa_amd_debug_round_flags(before)
            L.sa_amd_last_stats(ctypes.addressof(stats))
            st = stats.as_dict()
        return out, st, capfd.readouterr().err


def _rounds(err):
    return [(r["kind"], r.get("a", r.get("m")), r.get("b"), r.get("iters"), r.get("m_global")) for r in rm.parse_trace(err)]


def _check(oracle, monkeypatch, capfd, name, t, env):
    """the four builds of one text in one environment; returns the traces of modes 0 and 1"""
    exp = _oracle_sa(oracle, name, t)
    ref, st0, err0 = _build(monkeypatch, capfd, env, t, 0)
    assert np.array_equal(ref, exp), (env, name, "mode 0")
    assert BY_STATUS not in err0, (env, name)
    err1 = None
    for mode in (1, 2, None):
        got, st, err = _build(monkeypatch, capfd, env, t, mode)
        assert np.array_equal(got, exp), (env, name, mode)
        if t.size:      # (an empty text builds nothing: the last build's statistics stay, whichever library ran it)
            assert st == st0, (env, name, mode)
        assert _rounds(err) == _rounds(err0), (env, name, mode)
        if mode == 1:
            err1 = err
        elif mode is None:
            assert (BY_STATUS in err) == (BY_STATUS in err1), (env, name)
    return err0, err1


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES, ids=_IDS)
def test_builds_equal_the_key_route(oracle, monkeypatch, capfd, regime):
    taken, misses = 0, 0
    for name, t in _texts():
        # the adversarial cases are shorter than the one-workgroup path takes (8192 bytes): they run as they are and once more
        # through the general pipeline
        for extra in ({}, {"SA_AMD_SMALL_MAX": "0"}) if t.size <= 8192 else ({},):
            err0, err1 = _check(oracle, monkeypatch, capfd, name, t, dict(regime, **extra))
            taken += err1.count(BY_STATUS)
            misses += sum(int(x) for x in _MISSES.findall(err1))
            if name.startswith("list_of_") and "SA_AMD_FORCE_DENSE" in regime and (t.size > 8192 or extra):
                # the list the first doubling round refines has the length the text was made for
                first = [r for r in rm.parse_trace(err0) if r["kind"] == "doubling"][0]
                assert first["a"] == int(name[8:]), (name, first)
    assert taken > 0, regime
    print(f"rounds that read status bytes: {taken}; deferred rounds that missed: {misses}")


@pytest.mark.gpu
def test_keys_behind_text_rounds(oracle, monkeypatch, capfd):
    """default environment, a text that takes text-keyed rounds and then doubles densely: the third key buffer is a key buffer of
    the rounds there, no slab is free for the bytes, and the trace says that every dense round read keys"""
    blk = _rnd(700 * 7 + 97, 700)
    t = np.tile(blk, 97)
    err0, err1 = _check(oracle, monkeypatch, capfd, "blocks_700x97_default", t, {})
    kinds = [r["kind"] for r in rm.parse_trace(err1)]
    assert "text" in kinds and "doubling" in kinds, kinds
    assert kinds.index("text") < kinds.index("doubling")
    assert BY_KEYS in err1 and BY_STATUS not in err1, err1
    # ... and straight from the initial order the same text takes the bytes
    _, err1 = _check(oracle, monkeypatch, capfd, "blocks_700x97_default", t, {"SA_AMD_FORCE_DENSE": "1"})
    assert BY_STATUS in err1, err1


@pytest.mark.gpu
def test_status_bytes_on_device_pointers(oracle, monkeypatch):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    t = corpus.english_corpus(1 << 20, 13)
    exp = oracle.sais(t)
    n = int(t.size)
    wb = sa.workspace_bytes(n)
    dt, do, dw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dt), n + 64) == 0 and hip.hipMalloc(ctypes.byref(do), 4 * (n + 1) + 64) == 0
    assert hip.hipMalloc(ctypes.byref(dw), wb + 512) == 0
    try:
        assert hip.hipMemcpy(dt.value, t.ctypes.data, n, 1) == 0
        D = sa.diag_lib()
        for regime in ({"SA_AMD_FORCE_DENSE": "1"}, {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"}):
            stats = []
            for L, m in ((D, 0), (D, 1), (D, 2), (sa.lib(), None)):
                out = np.zeros(n + 1, dtype=np.uint32)
                st = sa.Stats()
                before = D.sa_amd_debug_round_flags(m if m is not None else 1)
                try:
                    with monkeypatch.context() as mp:
                        for k, v in regime.items():
                            mp.setenv(k, v)
                        rc = L.sa_amd_saca_device(dt.value, do.value, n, (dw.value + 255) & ~255, wb, None, ctypes.addressof(st))
                finally:
                    D.sa_amd_debug_round_flags(before)
                assert rc == 0
                assert hip.hipMemcpy(out.ctypes.data, do.value, 4 * (n + 1), 2) == 0
                assert np.array_equal(out, exp), (regime, m)
                stats.append(st.as_dict())
            assert stats[0] == stats[1] == stats[2] == stats[3], (regime, stats)
    finally:
        for ptr in (dt, do, dw):
            hip.hipFree(ptr)


@pytest.mark.gpu
def test_keys_on_the_reduced_memory_route(oracle, monkeypatch, capfd):
    """another tenant holds nearly all of the HBM (as in test_reduced_memory_route_when_the_device_is_nearly_full): the third key
    buffer, the last slab of the workspace, is in pinned host memory -- the rounds keep their keys, and the array is the oracle's"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    t = corpus.english_corpus(40 << 20, 6)
    exp = oracle.sais(t)
    sa.lib().sa_amd_release_cache()
    need = int(t.size) * 5 + sa.workspace_bytes(int(t.size))
    f, tot = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(tot)) == 0
    hog = ctypes.c_void_p()
    leave = int(need * 0.85)             # the whole workspace does not fit: its last slabs, the third key buffer among them, go to the host
    assert hip.hipMalloc(ctypes.byref(hog), int(f.value) - leave) == 0
    try:
        out = np.zeros(t.size + 1, dtype=np.uint32)
        monkeypatch.setenv("SA_AMD_FORCE_DENSE", "1")
        monkeypatch.setenv("SA_AMD_VERBOSE", "3")
        capfd.readouterr()
        sa.saca(t, out)
        err = capfd.readouterr().err
        assert sa.last_host_timing()["workspace_bytes_in_host_memory"] > 0
        assert np.array_equal(out, exp)
        assert BY_KEYS in err and BY_STATUS not in err, err
    finally:
        hip.hipFree(hog)
        sa.lib().sa_amd_release_cache()
