"""The dense route's re-rank writes: SA written once per slot, in the round its suffix leaves the tied list (k_rr_apply sa_final),
and the binned rank set-up reading its pair keys from the suffix array itself.  The old forms (every listed slot in every round; a
copy of SA as the pair keys) are switched on by sa_amd_debug_rerank_routes of the diagnostic library, which is built from the same
sources.  Every route is checked against the old one and against the oracle, and the product library against both."""
import ctypes
import os

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ROUTES = [0, 1, 2, 3]      # sa_amd_debug_rerank_routes flags: bit 0 = SA every round, bit 1 = set-up keys copied; 3 = the old form
OLD = 3

# regimes that reach the dense rounds and the binned set-up at small sizes
REGIMES = [
    {"SA_AMD_FORCE_DENSE": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1", "SA_AMD_SCATTER_LEVELS": "2"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1", "SA_AMD_SCATTER_LEVELS": "1", "SA_AMD_NO_TOP32": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1", "SA_AMD_NO_FIRST_TAIL": "1", "SA_AMD_NO_LOCAL_SORT": "1"},
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_MIN": "1", "SA_AMD_DENSE_REKEY_MIN": "1", "SA_AMD_GROUP_CAP": "16"},
    # the early download reads SA while the rounds run: it must only take slots outside the tied list
    {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1", "SA_AMD_STAGED_MIN_BYTES": "0", "SA_AMD_EARLY_MIN_BYTES": "0",
     "SA_AMD_EARLY_CHUNK_BYTES": "65536", "SA_AMD_EARLY_DIV": "1", "SA_AMD_EARLY_WAIT_CHUNKS": "1"},
    {},
]


def _build(text):
    return sa.SuffixArray(text).into_parts()[1]


def _diag():
    L = sa.diag_lib()
    L.sa_amd_debug_rerank_routes.argtypes = [ctypes.c_int32]
    L.sa_amd_debug_rerank_routes.restype = ctypes.c_int32
    L.sa_amd_saca_u8.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    L.sa_amd_saca_u8.restype = ctypes.c_int32
    L.sa_amd_saca_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.sa_amd_saca_device.restype = ctypes.c_int32
    return L


def _build_route(text, route):
    """the host-pointer entry point of the diagnostic library with the re-rank writes of `route`"""
    L = _diag()
    t = np.ascontiguousarray(text)
    out = np.zeros(t.size + 1, dtype=np.uint32)
    L.sa_amd_debug_rerank_routes(route)
    try:
        assert L.sa_amd_saca_u8(t.ctypes.data if t.size else None, out.ctypes.data, t.size) == 0
    finally:
        L.sa_amd_debug_rerank_routes(0)
    return out


def _with_env(monkeypatch, env, fn):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _golden_texts():
    out = []
    for f in sorted(os.listdir(GOLDEN)):
        if f.endswith(".text"):
            t = np.fromfile(os.path.join(GOLDEN, f), dtype=np.uint8)
            e = np.fromfile(os.path.join(GOLDEN, f[:-5] + ".sa.u32le"), dtype="<u4")
            out.append((f, t, e))
    return out


@pytest.mark.gpu
def test_routes_on_goldens_and_adversarial_cases(oracle, monkeypatch):
    cases = [(name, t, e) for name, t, e in _golden_texts()]
    for name, b in adversarial_cases().items():
        t = np.frombuffer(b, dtype=np.uint8).copy()
        cases.append((name, t, oracle.sais(t)))
    t = np.frombuffer(fibonacci_word(24)[:100_000], dtype=np.uint8).copy()
    cases.append(("fib", t, oracle.sais(t)))
    for regime in REGIMES:
        got = _with_env(monkeypatch, regime, lambda: [_build(t) for _, t, _ in cases])
        for (name, _, e), g in zip(cases, got):
            assert np.array_equal(g, e), (regime, name)
        for route in ROUTES:
            got = _with_env(monkeypatch, regime, lambda: [_build_route(t, route) for _, t, _ in cases])
            for (name, _, e), g in zip(cases, got):
                assert np.array_equal(g, e), (regime, route, name)


@pytest.mark.gpu
@pytest.mark.parametrize("mib", [1, 8, 64])
def test_routes_match_the_old_route_on_large_texts(oracle, monkeypatch, mib):
    n = mib << 20
    texts = [corpus.english_corpus(n, 7), np.concatenate([corpus.english(n // 2, 9)] * 2)]
    if mib <= 8:
        texts.append(corpus.dna_repeats(n, 3))
    regimes = [{}, {"SA_AMD_FORCE_DENSE": "1"}] if mib == 64 else REGIMES
    for t in texts:
        exp = oracle.sais(t)
        for regime in regimes:
            old = _with_env(monkeypatch, regime, lambda: _build_route(t, OLD))
            assert np.array_equal(old, exp), (regime, "old", t.size)
            assert np.array_equal(_with_env(monkeypatch, regime, lambda: _build(t)), old), (regime, "product", t.size)
            for route in ROUTES[:-1]:
                got = _with_env(monkeypatch, regime, lambda: _build_route(t, route))
                assert np.array_equal(got, old), (regime, route, t.size)


@pytest.mark.gpu
def test_routes_on_device_pointers(oracle, monkeypatch):
    """the device entry point (no early download): the array is complete when the call returns; an output that is not 16-byte
    aligned makes the set-up fall back to the copy of SA as pair keys"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    t = corpus.english_corpus(4 << 20, 13)
    exp = oracle.sais(t)
    n = int(t.size)
    wb = sa.workspace_bytes(n)
    dt, do, dw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dt), n + 64) == 0 and hip.hipMalloc(ctypes.byref(do), 4 * (n + 1) + 64) == 0
    assert hip.hipMalloc(ctypes.byref(dw), wb + 512) == 0
    L = _diag()
    try:
        assert hip.hipMemcpy(dt.value, t.ctypes.data, n, 1) == 0
        for shift in (0, 4):
            for regime in REGIMES[:3]:
                for route in ROUTES:
                    out = np.zeros(n + 1, dtype=np.uint32)
                    dst = do.value + shift
                    L.sa_amd_debug_rerank_routes(route)
                    try:
                        rc = _with_env(monkeypatch, regime,
                                       lambda: L.sa_amd_saca_device(dt.value, dst, n, (dw.value + 255) & ~255, wb, None, None))
                    finally:
                        L.sa_amd_debug_rerank_routes(0)
                    assert rc == 0
                    assert hip.hipMemcpy(out.ctypes.data, dst, 4 * (n + 1), 2) == 0
                    assert np.array_equal(out, exp), (shift, regime, route)
    finally:
        for ptr in (dt, do, dw):
            hip.hipFree(ptr)
