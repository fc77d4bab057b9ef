"""Group-start flags from the last pass of the 64-bit initial sort (k_onesweep<..., HEAD_FLAGS>, kernels/onesweep.hpp) and the
first re-rank that reads them instead of the sorted keys (rr_wave_classify_flags, kernels/rerank.hpp).

1. the pass alone, through sa_amd_test_sort_pairs_flags of the diagnostic library, against numpy;
2. whole builds against the oracle and against the key route: arrays and statistics must be equal;
3. the rebuild path (flags were written, the route taken reads the sorted keys);
4. the device-pointer entry point.

The product library has no switch: it writes flags when it expects the dense route (mode 1).  The diagnostic library, built from
the same sources, takes the mode from sa_amd_debug_head_flags: 0 = never (the key route, what the parent commit did), 1, 2 = always.
Every build below runs in the diagnostic library under each mode compared, and in the product library."""
import ctypes
import functools

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word

TILE = 8192
# the smallest shapes where tile, segment and ragged handling differ (tiles are 8192 elements, 4096 for shape 2)
COUNTS = [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 9 * TILE, 65536 + 17]
END_BITS = [61, 64, 40]          # last digits of 5, 8 and 8 bits
KEY_SETS = ["all_equal", "top_digit_cycling", "digit_in_first_and_last_tile", "thousand_values", "all_distinct"]


def _last_digit(end_bit):
    shift = 8 * ((end_bit + 7) // 8 - 1)
    return shift, end_bit - shift


@functools.lru_cache(maxsize=None)
def _case(kind, count, end_bit):
    """(keys, stable argsort, sorted keys); every key is below 2^end_bit, so the masked key is the key"""
    mask = np.uint64((1 << end_bit) - 1)
    shift, nb = _last_digit(end_bit)
    i = np.arange(count, dtype=np.uint64)
    if kind == "all_equal":
        keys = np.full(count, 0x0123456789ABCDEF, dtype=np.uint64)
    elif kind == "top_digit_cycling":
        # every tile holds every value of the last digit; the keys of one digit are all equal: one group per digit, across every seam
        keys = ((i % np.uint64(1 << nb)) << np.uint64(shift)) | np.uint64(0x5A5A5A)
    elif kind == "digit_in_first_and_last_tile":
        # digit 1 everywhere (a few distinct keys); digit 3 only in the first five and the last seven positions: the first run of
        # digit 3 in the last tile has its predecessor many tiles and segments back -- equal to it for some keys, larger for others
        one, three = np.uint64(1) << np.uint64(shift), np.uint64(3) << np.uint64(shift)
        keys = one | (i % np.uint64(7))
        keys[:5] = three | np.uint64(9)
        tail = min(7, max(count - 5, 0))
        if tail:
            keys[count - tail:] = three | np.uint64(9)
            keys[count - (tail + 1) // 2:] = three | np.uint64(10)
    elif kind == "thousand_values":
        rng = np.random.default_rng(1000 + end_bit)
        vals = rng.integers(0, 1 << 61, size=1000, dtype=np.uint64)
        keys = vals[rng.integers(0, 1000, size=count)]
    else:
        keys = i * np.uint64(0x9E3779B97F4A7C15)          # an odd multiplier: distinct modulo every power of two
    keys = np.ascontiguousarray(keys & mask)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    return keys, order, keys[order]


def _sort_flags(keys, end_bit):
    n = keys.size
    vals = np.arange(n, dtype=np.uint32)
    flags = np.full(n, 0xEE, dtype=np.uint8)
    kout = np.zeros(n, dtype=np.uint64)
    rc = sa.diag_lib().sa_amd_test_sort_pairs_flags(keys.ctypes.data, vals.ctypes.data, n, 0, end_bit, flags.ctypes.data, kout.ctypes.data)
    assert rc == 0
    return vals, flags, kout


@pytest.mark.gpu
@pytest.mark.parametrize("upfront", [True, False])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_flags_pass_against_numpy(monkeypatch, shape, upfront):
    monkeypatch.setenv("SA_AMD_ONESWEEP64_SHAPE", str(shape))
    if not upfront:
        monkeypatch.setenv("SA_AMD_NO_UPFRONT_COUNTS", "1")     # counts in the pass: up to eight segments
    for end_bit in END_BITS:
        for kind in KEY_SETS:
            for count in COUNTS:
                keys, order, ks = _case(kind, count, end_bit)
                vals, flags, kout = _sort_flags(keys, end_bit)
                where = (shape, upfront, end_bit, kind, count)
                assert np.array_equal(vals, order), where
                assert np.isin(flags, (0, 1, 2)).all(), where
                start = np.ones(count, dtype=bool)
                start[1:] = ks[1:] != ks[:-1]
                seam = np.flatnonzero(flags == 2)
                assert (seam > 0).all(), where                                    # (position 0 is a plain start)
                assert np.array_equal(kout[seam], ks[seam]), where                # both keys of a seam are true sorted keys
                assert np.array_equal(kout[seam - 1], ks[seam - 1]), where
                resolved = flags == 1
                resolved[seam] = kout[seam] != kout[seam - 1]
                assert np.array_equal(resolved, start), where


# ---- whole builds ----------------------------------------------------------------------------------------------------------

REGIMES = [
    {"SA_AMD_FORCE_DENSE": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_FIRST_TAIL": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_ONESWEEP64_SHAPE": "0"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_ONESWEEP64_SHAPE": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_ONESWEEP64_SHAPE": "2"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_KEY_BITS": "40"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_KEY_BITS": "64"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_GRAM_KEYS": "1"},
    {"SA_AMD_NO_TEXT_ROUNDS": "1"},
]
REBUILD_REGIMES = [{}, {"SA_AMD_SPARSE_DIV": "1"}]


@functools.lru_cache(maxsize=None)
def _texts():
    out = [(name, np.frombuffer(b, dtype=np.uint8).copy()) for name, b in adversarial_cases().items()]
    out.append(("fibonacci", np.frombuffer(fibonacci_word(24)[:100_000], dtype=np.uint8).copy()))
    for n in (8193, 65537, (1 << 20) + 3):
        out.append((f"english_{n}", corpus.english(n, 5)))
    block = corpus.english(8192, 11)
    out.append(("period_8192", np.concatenate([block] * 5 + [block[:7]])))       # equal keys on every tile seam
    out.append(("one_byte_value", np.full(20000, 0x61, dtype=np.uint8)))
    return tuple(out)


_expected = {}


def _oracle_sa(oracle, name, t):
    if name not in _expected:
        _expected[name] = oracle.sais(t)
    return _expected[name]


def _build(monkeypatch, env, t, mode=None):
    """(array, statistics) of one host-pointer build: mode None = the product library, else the diagnostic library in that mode"""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        if mode is None:
            return sa.SuffixArray(t).into_parts()[1], sa.last_stats()
        L = sa.diag_lib()
        t = np.ascontiguousarray(t)
        out = np.zeros(t.size + 1, dtype=np.uint32)
        st = sa.Stats()
        before = L.sa_amd_debug_head_flags(mode)
        try:
            assert L.sa_amd_saca_u8(t.ctypes.data if t.size else None, out.ctypes.data, t.size) == 0
        finally:
            L.sa_amd_debug_head_flags(before)
        L.sa_amd_last_stats(ctypes.addressof(st))
        return out, st.as_dict()


def _check_against_key_route(oracle, monkeypatch, regime, mode):
    # the adversarial cases are shorter than the one-workgroup path takes (8192 bytes): they run as they are and once more
    # through the general pipeline
    for name, t in _texts():
        exp = _oracle_sa(oracle, name, t)
        for extra in ({}, {"SA_AMD_SMALL_MAX": "0"}) if t.size <= 8192 else ({},):
            env = dict(regime, **extra)
            got, st = _build(monkeypatch, env, t, mode)
            ref, st0 = _build(monkeypatch, env, t, 0)
            prod, stp = _build(monkeypatch, env, t)
            assert np.array_equal(ref, exp), (env, name, "key route")
            assert np.array_equal(got, exp), (env, name, "flags")
            assert np.array_equal(prod, exp), (env, name, "product library")
            if t.size:      # (an empty text builds nothing: the last build's statistics stay, whichever library ran it)
                assert st == st0 and stp == st0, (env, name)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES, ids=lambda r: ",".join(f"{k[7:]}={v}" for k, v in r.items()))
def test_builds_equal_the_key_route(oracle, monkeypatch, regime):
    _check_against_key_route(oracle, monkeypatch, regime, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REBUILD_REGIMES, ids=["default_route", "sparse_route"])
def test_rebuild_path_equals_the_key_route(oracle, monkeypatch, regime):
    """flags are written whatever the probes say; the text rounds and the sparse rounds then get their sorted keys rebuilt"""
    _check_against_key_route(oracle, monkeypatch, regime, 2)


@pytest.mark.gpu
def test_the_flags_route_is_taken(monkeypatch, capfd):
    """the trace names the route: flags on the forced dense route (product library too), flags + rebuilt keys in mode 2 on a text
    that takes text rounds, neither in mode 0 or on that text by default"""
    t = corpus.english(65537, 5)
    wrote, rebuilt = "the last pass wrote group-start flags", "sorted keys rebuilt from the suffix array"
    for env, mode, want_flags, want_rebuild in (({"SA_AMD_FORCE_DENSE": "1"}, None, True, False),
                                                ({"SA_AMD_FORCE_DENSE": "1"}, 1, True, False),
                                                ({}, 2, True, True),
                                                ({"SA_AMD_FORCE_DENSE": "1"}, 0, False, False),
                                                ({}, 1, False, False),
                                                ({}, None, False, False)):
        capfd.readouterr()
        _build(monkeypatch, dict(env, SA_AMD_VERBOSE="3"), t, mode)
        err = capfd.readouterr().err
        assert (wrote in err) == want_flags, (env, mode, err)
        assert (rebuilt in err) == want_rebuild, (env, mode, err)


@pytest.mark.gpu
def test_flags_on_device_pointers(oracle, monkeypatch):
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
        for regime, mode in (({"SA_AMD_FORCE_DENSE": "1"}, 1), ({"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"}, 1), ({}, 2)):
            stats = []
            for L, m in ((D, 0), (D, mode), (sa.lib(), None)):
                out = np.zeros(n + 1, dtype=np.uint32)
                st = sa.Stats()
                before = D.sa_amd_debug_head_flags(m if m is not None else 1)
                try:
                    with monkeypatch.context() as mp:
                        for k, v in regime.items():
                            mp.setenv(k, v)
                        rc = L.sa_amd_saca_device(dt.value, do.value, n, (dw.value + 255) & ~255, wb, None, ctypes.addressof(st))
                finally:
                    D.sa_amd_debug_head_flags(before)
                assert rc == 0
                assert hip.hipMemcpy(out.ctypes.data, do.value, 4 * (n + 1), 2) == 0
                assert np.array_equal(out, exp), (regime, m)
                stats.append(st.as_dict())
            assert stats[0] == stats[1] == stats[2], (regime, stats)
    finally:
        for ptr in (dt, do, dw):
            hip.hipFree(ptr)
