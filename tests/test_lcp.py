"""GPU suite for the LCP array (kernels/lcp.hpp, host/lcp.hpp): every route against the oracle's Kasai, the boundaries of the
per-lane compare cap and of the binned Φ scatter, long-LCP families with the work bound asserted, the top of the size range
and the argument checks.  At most two large texts are alive at once."""
import ctypes
import math

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word

pytestmark = pytest.mark.gpu

CAP_DEFAULT, CAP_MAX = 64, 1 << 20
N_ABOVE = (1 << 30) + 4097

KNOWN = [
    (b"banana", [0, 0, 1, 3, 0, 0, 2]),
    (b"mississippi", [0, 0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3]),
    (b"splendid splendor", [0, 0, 0, 1, 1, 0, 3, 0, 0, 4, 0, 2, 0, 0, 5, 0, 0, 6]),
    (b"", [0]), (b"a", [0, 0]), (b"ab", [0, 0, 0]), (b"aa", [0, 0, 1]),
]


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def kasai(oracle, t, arr):
    L = oracle.L
    L.oracle_lcp_kasai.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.oracle_lcp_kasai.restype = ctypes.c_int32
    out = np.zeros(t.size + 1, dtype=np.uint32)
    a = np.ascontiguousarray(arr, dtype=np.uint32)
    assert L.oracle_lcp_kasai(t.ctypes.data, t.size, a.ctypes.data, out.ctypes.data) == 0
    return out


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")                       # (already in the process: the product library links it)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    return hip


class _Dev:
    """device buffers by hipMalloc (256-byte aligned), freed on exit"""

    def __init__(self, *sizes):
        self.hip = _hip()
        self.p = []
        for size in sizes:
            q = ctypes.c_void_p()
            assert self.hip.hipMalloc(ctypes.byref(q), max(int(size), 1)) == 0
            self.p.append(q.value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for q in self.p:
            self.hip.hipFree(q)


def lcp_on_device(t, arr, offset=0):
    """sa_amd_lcp_device on hipMalloc'ed buffers; `offset` bytes of misalignment in front of the text"""
    n = t.size
    wb = sa.lcp_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), 4 * (n + 1), wb) as d:
        dT, dS, dL, dW = d.p
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        sa.lcp_device_ptr(dT + offset, dS, n, dL, dW, wb)
        out = np.zeros(n + 1, dtype=np.uint32)
        assert d.hip.hipMemcpy(out.ctypes.data, dL, 4 * (n + 1), 2) == 0
    return out


def all_routes(t):
    """lcp, saca_lcp, lcp_device_ptr, DeviceIndex.lcp; all must agree; saca_lcp's array must be saca's"""
    arr = np.empty(t.size + 1, dtype=np.uint32)
    sa.saca(t, arr)
    a = sa.lcp(t, arr)
    arr2, b = sa.saca_lcp(t)
    assert np.array_equal(arr2, arr)
    c = lcp_on_device(t, arr)
    ix = sa.DeviceIndex(t, arr)
    d = ix.lcp()
    ix.close()
    for x in (b, c, d):
        assert np.array_equal(a, x)
    return arr, a


def work_bound(n):
    n = max(n, 2)
    return 2 * n * math.log2(n) + 32 * n


@pytest.mark.parametrize("text,expected", KNOWN)
def test_known_answers(text, expected):
    t = _u8(text)
    arr, got = all_routes(t)
    assert got.tolist() == expected


def test_run_of_equal_bytes_known_answer():
    t = np.full(1000, 0x61, dtype=np.uint8)
    _, got = all_routes(t)
    assert got[0] == 0 and np.array_equal(got[1:], np.arange(1000, dtype=np.uint32))


def test_adversarial_cases_all_routes(oracle):
    for name, b in adversarial_cases().items():
        t = _u8(b)
        arr, got = all_routes(t)
        assert np.array_equal(got, kasai(oracle, t, arr)), name


def test_golden_fixtures(oracle):
    import glob
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    files = sorted(glob.glob(os.path.join(here, "*.text")))
    assert files
    for f in files:
        t = np.fromfile(f, dtype=np.uint8)
        arr = np.fromfile(f[:-len(".text")] + ".sa.u32le", dtype="<u4").astype(np.uint32)
        exp = kasai(oracle, t, arr)
        assert np.array_equal(sa.lcp(t, arr), exp), f
        _, got = all_routes(t)
        assert np.array_equal(got, exp), f


def test_random_lengths(oracle):
    rng = np.random.default_rng(17)
    for k, n in enumerate(rng.integers(1, 20000, 24)):
        sigma = [2, 4, 26, 256][k % 4]
        t = rng.integers(0, sigma, int(n), dtype=np.uint8)
        arr, got = all_routes(t)
        assert np.array_equal(got, kasai(oracle, t, arr)), (n, sigma)


@pytest.mark.parametrize("cap", [None, 0, 1, 4, 5, 63, CAP_MAX])
def test_runs_around_the_compare_cap(oracle, cap):
    prev = sa.lcp_set_compare_cap(-1 if cap is None else cap)
    try:
        _runs_around_the_cap(oracle, cap)
    finally:
        sa.lcp_set_compare_cap(prev)


def _runs_around_the_cap(oracle, cap):
    c = CAP_DEFAULT if cap is None else cap
    rng = np.random.default_rng(c + 3)
    for k in sorted({max(c - 1, 1), max(c, 1), c + 1, 2 * c + 5}):
        if k > 70000:
            continue
        for t in (np.full(k, 9, dtype=np.uint8), np.frombuffer(b"x" * k + b"y" + b"x" * k, dtype=np.uint8),
                  np.concatenate([rng.integers(0, 4, k, dtype=np.uint8)] * 2)):
            arr = oracle.sais(t)
            got = sa.lcp(t, arr)
            assert np.array_equal(got, kasai(oracle, t, arr)), (cap, k)
            assert sa.last_lcp_stats()["compared_bytes"] <= work_bound(t.size)
    t = corpus.english_corpus(300000, 5)
    arr = oracle.sais(t)
    assert np.array_equal(sa.lcp(t, arr), kasai(oracle, t, arr)), cap
    if cap == 0:
        st = sa.last_lcp_stats()
        assert st["long_pairs"] > 0 and st["long_pairs"] <= st["irreducible"]


@pytest.mark.parametrize("knob", ["SA_AMD_BINNED_ISA_ALWAYS", "SA_AMD_NO_BINNED_ISA"])
def test_binned_phi_forced(oracle, monkeypatch, knob):
    monkeypatch.setenv(knob, "1")
    rng = np.random.default_rng(23)
    for t in (rng.integers(0, 256, 5000, dtype=np.uint8), corpus.dna(3 << 20, 2), corpus.english_corpus(1 << 20, 4),
              np.frombuffer(fibonacci_word(20), dtype=np.uint8)):
        arr = oracle.sais(t)
        assert np.array_equal(sa.lcp(t, arr), kasai(oracle, t, arr))
    monkeypatch.setenv("SA_AMD_SCATTER_LEVELS", "2")
    t = corpus.english_corpus(1 << 20, 6)
    arr = oracle.sais(t)
    assert np.array_equal(sa.lcp(t, arr), kasai(oracle, t, arr))


@pytest.mark.parametrize("mib", [16, 64])
@pytest.mark.parametrize("name", ["uniform", "dna", "dna_repeats", "english_corpus"])
def test_corpora_against_kasai(oracle, name, mib):
    n = mib << 20
    t = getattr(corpus, name)(n, 7)
    arr, got = sa.saca_lcp(t)
    assert np.array_equal(got, kasai(oracle, t, arr))
    assert sa.last_lcp_stats()["compared_bytes"] <= work_bound(n)


def _fib_text(n):
    k, w = 1, fibonacci_word(1)
    while len(w) < n:
        k += 1
        w = fibonacci_word(k)
    return np.frombuffer(w[:n], dtype=np.uint8)


@pytest.mark.parametrize("family", ["one_byte", "period2", "twice", "fibonacci"])
def test_long_lcp_families_64m(oracle, family):
    n = 64 << 20
    if family == "one_byte":
        t = np.full(n, 0x41, dtype=np.uint8)
        arr = np.arange(n, -1, -1, dtype=np.uint32)                  # closed form: SA = [n, n-1, ..., 0]
        got = sa.lcp(t, arr)
        assert got[0] == 0 and np.array_equal(got[1:], np.arange(n, dtype=np.uint32))
    else:
        if family == "period2":
            t = np.tile(np.array([1, 2], dtype=np.uint8), n // 2)
        elif family == "twice":
            h = corpus.uniform(n // 2, 9)
            t = np.concatenate([h, h])
        else:
            t = _fib_text(n)
        arr, got = sa.saca_lcp(t)
        assert np.array_equal(got, kasai(oracle, t, arr)), family
    st = sa.last_lcp_stats()
    assert st["compared_bytes"] <= work_bound(n), (family, st)


def _sampled_lcp_ok(t, arr, got, seed, samples=3000):
    rng = np.random.default_rng(seed)
    n = t.size
    for i in rng.integers(1, n + 1, samples):
        a, b, h = int(arr[i - 1]), int(arr[i]), int(got[i])
        x, y = t[a:a + h + 1], t[b:b + h + 1]
        assert np.array_equal(x[:h], y[:h]), (i, a, b, h)
        assert x.size == h or y.size == h or x[h] != y[h], (i, a, b, h)


def test_top_of_range_one_byte_closed_form():
    n = N_ABOVE
    t = np.full(n, 0x7A, dtype=np.uint8)
    arr = np.arange(n, -1, -1, dtype=np.uint32)
    got = sa.lcp(t, arr)
    del arr
    assert got[0] == 0
    step = 1 << 26
    for s in range(1, n + 1, step):
        e = min(s + step, n + 1)
        assert np.array_equal(got[s:e], np.arange(s - 1, e - 1, dtype=np.uint32)), s
    st = sa.last_lcp_stats()
    assert st["long_pairs"] == 1 and st["compared_bytes"] <= 4 * n
    del got, t
    sa.lib().sa_amd_release_cache()


def test_top_of_range_uniform_sampled():
    n = N_ABOVE
    t = corpus.uniform(n, 31)
    arr, got = sa.saca_lcp(t)
    assert arr[0] == n and got[0] == 0 and got[1] == 0
    _sampled_lcp_ok(t, arr, got, 41)
    assert int(got.max()) < 64
    del arr, got, t
    sa.lib().sa_amd_release_cache()


def test_closed_form_array_then_lcp(monkeypatch):
    monkeypatch.delenv("SA_AMD_NO_UNARY_SHORTCUT", raising=False)
    n = (1 << 20) + 3
    t = np.full(n, 0xEE, dtype=np.uint8)
    arr, got = sa.saca_lcp(t)
    assert np.array_equal(arr, np.arange(n, -1, -1, dtype=np.uint32))
    assert got[0] == 0 and np.array_equal(got[1:], np.arange(n, dtype=np.uint32))


def test_errors():
    L = sa.lib()
    t = _u8(b"mississippi")
    n = t.size
    arr = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, arr)
    out = np.zeros(n + 1, dtype=np.uint32)
    bad = arr.copy()
    bad[5] = n + 1
    assert L.sa_amd_lcp(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data) == -6
    with pytest.raises(IndexError):
        sa.lcp(t, bad)
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]
    assert L.sa_amd_lcp(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data) == -1
    assert L.sa_amd_lcp(None, n, arr.ctypes.data, out.ctypes.data) == -1
    assert L.sa_amd_lcp(t.ctypes.data, -1, arr.ctypes.data, out.ctypes.data) == -1
    assert L.sa_amd_lcp(t.ctypes.data, n, arr.ctypes.data, None) == -1
    zero = np.zeros(1, dtype=np.uint32)
    assert L.sa_amd_lcp(None, 0, np.array([1], dtype=np.uint32).ctypes.data, zero.ctypes.data) == -6
    assert L.sa_amd_lcp(None, 0, np.array([0], dtype=np.uint32).ctypes.data, zero.ctypes.data) == 0 and zero[0] == 0
    # the device entry point: a short work block is refused
    with _Dev(n, 4 * (n + 1), 4 * (n + 1), sa.lcp_work_bytes(n)) as d:
        dT, dS, dL, dW = d.p
        assert d.hip.hipMemcpy(dS, arr.ctypes.data, 4 * (n + 1), 1) == 0
        assert d.hip.hipMemcpy(dT, t.ctypes.data, n, 1) == 0
        assert L.sa_amd_lcp_device(dT, dS, n, dL, dW, 64, None) == -1
        assert L.sa_amd_lcp_device(dT, dS, n, dL, dW + 4, sa.lcp_work_bytes(n) - 256, None) == -1     # misaligned work block
        assert L.sa_amd_lcp_device(dT, dS, n, dL, dW, sa.lcp_work_bytes(n), None) == 0


def test_misaligned_text(oracle):
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 5, 7, 1000, 4099, 100003):
        t = rng.integers(0, 3, n, dtype=np.uint8)
        arr = oracle.sais(t)
        exp = kasai(oracle, t, arr)
        for off in (0, 1, 2, 3):
            assert np.array_equal(lcp_on_device(t, arr, off), exp), (n, off)


def test_profile_classes_report_lcp_kernels():
    L = sa.lib()
    names = []
    while True:
        nm = L.sa_amd_profile_kernel_name(len(names)).decode()
        if not nm:
            break
        names.append(nm)
    assert len(names) <= 32
    t = corpus.english_corpus(1 << 20, 8)
    arr = np.empty(t.size + 1, dtype=np.uint32)
    sa.saca(t, arr)
    L.sa_amd_profile_begin()
    sa.lcp(t, arr)
    cap = 32
    ms, launches, units = (ctypes.c_double * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
    cnt = L.sa_amd_profile_end(ms, launches, units, cap)
    got = {names[i]: launches[i] for i in range(cnt)}
    for k in ("k_lcp_phi", "k_lcp_irreducible", "k_lcp_scan", "k_lcp_gather"):
        assert got[k] > 0, (k, got)
    st = sa.last_lcp_stats()
    assert st["irreducible"] > 0 and st["readbacks"] >= 2


def test_suffix_array_lcp_array_extension(oracle):
    t = corpus.english(100000, 2)
    s = sa.SuffixArray(t)
    _, arr = s.into_parts()
    assert np.array_equal(s.lcp_array(), kasai(oracle, t, arr))
