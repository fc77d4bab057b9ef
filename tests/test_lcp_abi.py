"""CPU suite for the LCP array: the exports, the argument checks that answer without a device, and the algorithm itself
restated in numpy (permuted LCP: irreducible values compared directly, the rest by one max-scan) against the oracle's Kasai."""
import ctypes
import math

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import adversarial_cases, fibonacci_word

EXPORTS = ("sa_amd_lcp", "sa_amd_lcp_device", "sa_amd_lcp_work_bytes", "sa_amd_saca_u8_lcp", "sa_amd_index_lcp",
           "sa_amd_last_lcp_stats", "sa_amd_lcp_set_compare_cap")


def _kasai(oracle, t, arr):
    L = oracle.L
    L.oracle_lcp_kasai.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.oracle_lcp_kasai.restype = ctypes.c_int32
    out = np.zeros(t.size + 1, dtype=np.uint32)
    a = np.ascontiguousarray(arr, dtype=np.uint32)
    assert L.oracle_lcp_kasai(t.ctypes.data, t.size, a.ctypes.data, out.ctypes.data) == 0
    return out


def plcp_model(t, arr):
    """kernels/lcp.hpp in numpy: Φ, irreducible values by direct comparison, v = j + h, max-scan, gather.
    Returns (lcp, sum of the irreducible values)."""
    n = t.size
    if n == 0:
        return np.zeros(1, dtype=np.uint32), 0
    s = arr.astype(np.int64)
    phi = np.empty(n, dtype=np.int64)
    phi[s[1:]] = s[:-1]                                             # Φ[SA[i]] = SA[i-1]; Φ[SA[1]] = n
    j = np.arange(n)
    inner = (phi > 0) & (phi < n)
    red = (j > 0) & inner & (t[np.maximum(j - 1, 0)] == t[np.where(inner, phi - 1, 0)])
    v = np.zeros(n, dtype=np.int64)
    total = 0
    for k in np.nonzero(~red)[0]:
        p, h = int(phi[k]), 0
        if p != n:
            lim = n - max(int(k), p)
            while h < lim and t[k + h] == t[p + h]:
                h += 1
        total += h
        v[k] = k + h
    plcp = np.maximum.accumulate(v) - j                             # PLCP[j] + j never decreases
    lcp = np.zeros(n + 1, dtype=np.uint32)
    lcp[1:] = plcp[s[1:]]
    return lcp, total


def test_library_exports_the_lcp_entry_points():
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert hasattr(L, fn), fn
    assert hasattr(sa.lib(), "sa_amd_lcp")
    for name in ("lcp", "saca_lcp", "last_lcp_stats", "lcp_device_ptr"):
        assert callable(getattr(sa, name))
    assert callable(sa.DeviceIndex.lcp) and callable(sa.SuffixArray.lcp_array)


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.zeros(16, dtype=np.uint32)
    p = buf.ctypes.data
    assert L.sa_amd_lcp_work_bytes(-1) == -1
    assert L.sa_amd_lcp(None, -1, p, p) == -1                       # n < 0
    assert L.sa_amd_lcp(None, 4, p, p) == -1                        # null text
    assert L.sa_amd_lcp(p, 4, None, p) == -1                        # null array
    assert L.sa_amd_lcp(p, 4, p, None) == -1                        # null output
    assert L.sa_amd_saca_u8_lcp(p, p, -3, p) == -1
    assert L.sa_amd_saca_u8_lcp(p, None, 4, p) == -1
    assert L.sa_amd_saca_u8_lcp(p, p, 4, None) == -1
    assert L.sa_amd_lcp_device(p, p, -1, p, p, 1 << 20, None) == -1
    assert L.sa_amd_lcp_device(p, None, 4, p, p, 1 << 20, None) == -1
    assert L.sa_amd_lcp_device(p, p, 4, None, p, 1 << 20, None) == -1
    assert L.sa_amd_lcp_device(p, p, 4, p, None, 1 << 20, None) == -1
    assert L.sa_amd_lcp_device(None, p, 4, p, p, 1 << 20, None) == -1
    assert L.sa_amd_index_lcp(None, p) == -1
    st = sa.LcpStats()
    L.sa_amd_last_lcp_stats(ctypes.byref(st))                       # (no build on this thread yet: zeros, no device needed)
    L.sa_amd_last_lcp_stats(None)
    prev = sa.lcp_set_compare_cap(0)                                # (a thread-local route switch: no device involved)
    assert sa.lcp_set_compare_cap(1 << 30) == 0
    assert sa.lcp_set_compare_cap(-1) == 1 << 20                     # clamped to the maximum
    assert sa.lcp_set_compare_cap(prev) == 64


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 4096, 1 << 20, (1 << 30) + 4097, 2**31 - 1])
def test_work_block_within_the_integrity_checks(n):
    """the LCP work block is no larger than the streaming integrity check's plus 4 (n + 1) bytes"""
    L = sa.lib()
    w = L.sa_amd_lcp_work_bytes(n)
    assert 0 < w <= L.sa_amd_check_integrity_work_bytes(n) + 4 * (n + 1)
    assert w % 256 == 0


def test_model_matches_kasai_on_adversarial_cases(oracle):
    for name, b in adversarial_cases().items():
        t = np.frombuffer(b, dtype=np.uint8) if b else np.zeros(0, dtype=np.uint8)
        arr = oracle.sais(t)
        got, total = plcp_model(t, arr)
        assert np.array_equal(got, _kasai(oracle, t, arr)), name
        n = max(t.size, 2)
        assert total <= 2 * n * math.log2(n), name               # the work bound of the irreducible values


def test_model_on_long_lcp_families(oracle):
    rng = np.random.default_rng(5)
    half = rng.integers(0, 256, 3000, dtype=np.uint8)
    for name, t in (("fib", np.frombuffer(fibonacci_word(20), dtype=np.uint8)), ("twice", np.concatenate([half, half])),
                    ("period2", np.frombuffer(b"ab" * 3000, dtype=np.uint8)), ("run", np.full(3000, 7, dtype=np.uint8))):
        arr = oracle.sais(t)
        got, total = plcp_model(t, arr)
        assert np.array_equal(got, _kasai(oracle, t, arr)), name
        assert total <= 2 * t.size * math.log2(t.size), name
    run = np.full(300, 1, dtype=np.uint8)
    _, total = plcp_model(run, oracle.sais(run))
    assert total == 299                                             # one irreducible pair, h = n - 1 (Kasai's values sum to 44 850)
