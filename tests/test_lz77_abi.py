"""CPU suite for the Lempel-Ziv factorisation: the definitions of include/suffix_array_amd.h restated in numpy (LPF with its
sources, the greedy parse, decoding), checked against literal brute force and the known answers; the oracle library's
linear-time restatement (the reference of the GPU suite at sizes numpy does not reach) against the numpy one; the exports, the
Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases, fibonacci_word, thue_morse
from test_lcp_abi import _kasai

EXPORTS = ("sa_amd_lz_work_bytes", "sa_amd_lpf_device", "sa_amd_lz77_device", "sa_amd_lpf", "sa_amd_lz77", "sa_amd_index_lpf",
           "sa_amd_index_lz77", "sa_amd_last_lz_stats")
LIT = 0xFFFFFFFF


# ---------------------------------------------------------------- the definitions ----

def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def neighbour_slots(a):
    """stack pass over the values a[0 .. m): (psv, nsv), the nearest index to the left / right that holds a smaller value, -1
    where there is none"""
    a = np.asarray(a, dtype=np.int64).tolist()
    m = len(a)
    psv, nsv = [-1] * m, [-1] * m
    st = []
    for i in range(m):
        while st and a[st[-1]] > a[i]:
            nsv[st.pop()] = i
        if st:
            psv[i] = st[-1]
        st.append(i)
    return np.asarray(psv, dtype=np.int64), np.asarray(nsv, dtype=np.int64)


def partners(arr):
    """P, N in text order (n where there is none) from the suffix array in the layout of saca"""
    s = np.asarray(arr[1:], dtype=np.int64)
    n = s.size
    psv, nsv = neighbour_slots(s)
    P, N = np.full(n, n, dtype=np.int64), np.full(n, n, dtype=np.int64)
    P[s] = np.where(psv >= 0, s[np.maximum(psv, 0)], n)
    N[s] = np.where(nsv >= 0, s[np.maximum(nsv, 0)], n)
    return P, N


def _lcp_compare(t, p, q):
    """lcp(T[p..], T[q..]) by comparison, in pieces that double"""
    n = t.size
    lim = n - max(p, q)
    h, step = 0, 16
    while h < lim:
        k = min(step, lim - h)
        neq = np.nonzero(t[p + h:p + h + k] != t[q + h:q + h + k])[0]
        if neq.size:
            return h + int(neq[0])
        h += k
        step *= 2
    return lim


def _merge(lp, ln, P, N):
    lpf = np.maximum(lp, ln)
    src = np.where(lpf == 0, LIT, np.where(lp >= ln, P, N))
    return lpf.astype(np.int64), src.astype(np.int64)


def lpf_definition(t, arr):
    """(LPF, SRC): a stack pass over the suffix array for P and N, then lcp by comparison, then the tie rule"""
    t = _u8(t)
    n = t.size
    P, N = partners(arr)
    lp = np.array([0 if P[p] == n else _lcp_compare(t, p, int(P[p])) for p in range(n)], dtype=np.int64)
    ln = np.array([0 if N[p] == n else _lcp_compare(t, p, int(N[p])) for p in range(n)], dtype=np.int64)
    return _merge(lp, ln, P, N)


def lpf_from_lcp(t, arr, lcp):
    """the same for texts whose matches are too long to compare pair by pair: lcp(T[p..], T[q..]) is the minimum of the LCP array
    between the two slots (sparse table)"""
    t = _u8(t)
    n = t.size
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    s = np.asarray(arr[1:], dtype=np.int64)
    psv, nsv = neighbour_slots(s)
    lc = np.asarray(lcp[1:], dtype=np.int64)                         # lc[i] = lcp of 0-based slots i - 1 and i
    table = [lc]
    w = 1
    while 2 * w <= n:
        table.append(np.minimum(table[-1][:-w], table[-1][w:]))
        w *= 2

    def range_min(lo, hi):                                            # min lc[lo .. hi], lo <= hi (arrays)
        k = np.frexp((hi - lo + 1).astype(np.float64))[1] - 1
        out = np.empty(lo.size, dtype=np.int64)
        for lev in np.unique(k):
            sel = k == lev
            tb = table[lev]
            out[sel] = np.minimum(tb[lo[sel]], tb[hi[sel] - (1 << lev) + 1])
        return out

    i = np.arange(n, dtype=np.int64)
    lp_slot = np.zeros(n, dtype=np.int64)
    has = psv >= 0
    lp_slot[has] = range_min(psv[has] + 1, i[has])
    ln_slot = np.zeros(n, dtype=np.int64)
    has = nsv >= 0
    ln_slot[has] = range_min(i[has] + 1, nsv[has])
    lp, ln = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    lp[s], ln[s] = lp_slot, ln_slot
    P, N = partners(arr)
    return _merge(lp, ln, P, N)


def parse_definition(lpf, src):
    """the greedy parse: (z, 2) rows (SRC[s_k], max(1, LPF[s_k]))"""
    lpf, src = np.asarray(lpf, dtype=np.int64), np.asarray(src, dtype=np.int64)
    out, p = [], 0
    while p < lpf.size:
        ln = max(1, int(lpf[p]))
        out.append((int(src[p]), ln))
        p += ln
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def decode(phrases, t):
    """the text back from the phrases and the literal bytes of t"""
    return sa.lz77_decode(phrases, sa.lz77_literals(t, phrases))


def stats_definition(phrases):
    ph = np.asarray(phrases, dtype=np.int64).reshape(-1, 2)
    if ph.shape[0] == 0:
        return {"phrases": 0, "literals": 0, "longest": 0, "longest_pos": -1}
    starts = np.cumsum(ph[:, 1]) - ph[:, 1]
    longest = int(ph[:, 1].max())
    return {"phrases": int(ph.shape[0]), "literals": int(np.count_nonzero(ph[:, 0] == LIT)), "longest": longest,
            "longest_pos": int(starts[np.nonzero(ph[:, 1] == longest)[0][0]])}


def oracle_lz77(oracle, t, arr, capacity=None):
    """oracle_lz77 of oracle/oracle.c -> (LPF, SRC, the phrases that fit `capacity` (default: all), the number of all phrases), uint32"""
    L = oracle.L
    L.oracle_lz77.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    L.oracle_lz77.restype = ctypes.c_int64
    t = _u8(t)
    n = t.size
    a = np.ascontiguousarray(arr, dtype=np.uint32)
    assert a.size == n + 1
    capacity = n if capacity is None else capacity
    lpf, src = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    ph = np.full((capacity + 1, 2), 0xEEEEEEEE, dtype=np.uint32)
    z = L.oracle_lz77(t.ctypes.data, n, a.ctypes.data, lpf.ctypes.data, src.ctypes.data, ph.ctypes.data, capacity)
    assert z >= 0 and np.all(ph[min(z, capacity):] == 0xEEEEEEEE)
    return lpf, src, ph[:min(z, capacity)].copy(), z


def _fib_text(n):
    k, w = 1, fibonacci_word(1)
    while len(w) < n:
        k += 1
        w = fibonacci_word(k)
    return np.frombuffer(w[:n], dtype=np.uint8)


def _families(n, seed=1):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 256, n // 2, dtype=np.uint8)
    out = {
        "one_byte": np.full(n, 0x41, dtype=np.uint8), "period2": np.resize(np.array([1, 2], dtype=np.uint8), n),
        "fibonacci": _fib_text(n), "thue_morse": np.frombuffer(thue_morse(n), dtype=np.uint8),
        "twice": np.resize(np.concatenate([h, h]), n), "akbak": np.concatenate([np.full(n // 2, 97), [98], np.full(n - n // 2 - 1, 97)]),
        "random2": rng.integers(0, 2, n, dtype=np.uint8), "random4": rng.integers(0, 4, n, dtype=np.uint8),
        "random256": rng.integers(0, 256, n, dtype=np.uint8), "zeros_ffs": rng.choice(np.array([0, 0xFF], dtype=np.uint8), n),
    }
    return {k: np.ascontiguousarray(v[:n], dtype=np.uint8) for k, v in out.items()}


# ---------------------------------------------------------------- literal brute force ----

def brute_lpf(t):
    n = len(t)
    out = []
    for p in range(n):
        best = 0
        for q in range(p):
            h = 0
            while p + h < n and t[q + h] == t[p + h]:
                h += 1
            best = max(best, h)
        out.append(best)
    return out


def _sa_of(b):
    n = len(b)
    return np.array([n] + sorted(range(n), key=lambda i: b[i:]), dtype=np.uint32)


def test_definitions_against_brute_force(oracle):
    rng = np.random.default_rng(14)
    for trial in range(300):
        n = int(rng.integers(1, 41))
        b = bytes(rng.integers(0, int(rng.integers(1, 5)), n, dtype=np.uint8))
        t = _u8(b)
        arr = _sa_of(b)
        lpf, src = lpf_definition(t, arr)
        assert lpf.tolist() == brute_lpf(b), b
        for p in range(n):
            if lpf[p] == 0:
                assert src[p] == LIT
            else:
                q = int(src[p])
                assert q < p and b[q:q + lpf[p]] == b[p:p + lpf[p]], (b, p)
        assert np.all(lpf[1:] >= lpf[:-1] - 1)
        lpf2, src2 = lpf_from_lcp(t, arr, _kasai(oracle, t, arr))
        assert np.array_equal(lpf, lpf2) and np.array_equal(src, src2), b
        ph = parse_definition(lpf, src)
        assert int(ph[:, 1].sum()) == n and decode(ph, t) == b
        st = stats_definition(ph)
        assert st["phrases"] == ph.shape[0] and 1 <= st["longest"] <= n


def _oracle_equals_definitions(oracle, t, arr, name):
    t = _u8(t)
    lpf, src = lpf_from_lcp(t, arr, _kasai(oracle, t, arr))
    ph = parse_definition(lpf, src)
    glpf, gsrc, gph, z = oracle_lz77(oracle, t, arr)
    assert np.array_equal(glpf, lpf) and np.array_equal(gsrc, src), name
    assert z == ph.shape[0] and np.array_equal(gph, ph), name
    for cap in (0, z // 2, max(z - 1, 0)):                            # a cut capacity: the true count, the true prefix
        _, _, cut, zc = oracle_lz77(oracle, t, arr, cap)
        assert zc == z and np.array_equal(cut, ph[:cap]), (name, cap)


def test_oracle_lz77_equals_the_definitions(oracle):
    for name, b in adversarial_cases().items():
        t = _u8(b)
        _oracle_equals_definitions(oracle, t, oracle.sais(t), name)
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "manifest.json")) as f:
        names = sorted(json.load(f))
    assert names
    for name in names:
        t = np.fromfile(os.path.join(gold, name + ".text"), dtype=np.uint8)
        _oracle_equals_definitions(oracle, t, np.fromfile(os.path.join(gold, name + ".sa.u32le"), dtype="<u4"), name)
    for name, t in _families(3001).items():
        _oracle_equals_definitions(oracle, t, oracle.sais(t), name)
    assert oracle_lz77(oracle, b"banana", oracle.sais(b"banana"))[2].tolist() == [[LIT, 1], [LIT, 1], [LIT, 1], [1, 3]]


def test_known_answers():
    t = _u8(b"banana")
    arr = _sa_of(b"banana")
    lpf, src = lpf_definition(t, arr)
    assert lpf.tolist() == [0, 0, 0, 3, 2, 1] and src.tolist() == [LIT, LIT, LIT, 1, 2, 3]        # (SRC[5]: P(5) = n, N(5) = 3, ln = 1)
    ph = parse_definition(lpf, src)
    assert ph.tolist() == [[LIT, 1], [LIT, 1], [LIT, 1], [1, 3]]
    assert sa.lz77_literals(t, ph) == b"ban" and sa.lz77_decode(ph, b"ban") == b"banana"
    assert stats_definition(ph) == {"phrases": 4, "literals": 3, "longest": 3, "longest_pos": 3}
    for n in (1, 2, 3, 50):                                           # one byte: {(LIT, 1), (0, n - 1)}, the copy overlaps itself
        b = b"a" * n
        lpf, src = lpf_definition(_u8(b), _sa_of(b))
        assert lpf.tolist() == [0] + list(range(n - 1, 0, -1))
        ph = parse_definition(lpf, src)
        assert ph.tolist() == ([[LIT, 1], [0, n - 1]] if n > 1 else [[LIT, 1]]) and decode(ph, _u8(b)) == b
    b = b"ab" * 20
    lpf, src = lpf_definition(_u8(b), _sa_of(b))
    assert parse_definition(lpf, src).tolist() == [[LIT, 1], [LIT, 1], [0, 38]]
    assert parse_definition([], []).shape == (0, 2) and sa.lz77_decode(np.zeros((0, 2)), b"") == b""


def test_neighbour_slots():
    psv, nsv = neighbour_slots([3, 1, 4, 0, 5, 9, 2, 6])
    assert psv.tolist() == [-1, -1, 1, -1, 3, 4, 3, 6] and nsv.tolist() == [1, 3, 3, -1, 6, 6, -1, -1]
    m = 200
    rng = np.random.default_rng(3)
    a = rng.permutation(m)
    psv, nsv = neighbour_slots(a)
    for i in range(m):
        left = [j for j in range(i) if a[j] < a[i]]
        right = [j for j in range(i + 1, m) if a[j] < a[i]]
        assert psv[i] == (left[-1] if left else -1) and nsv[i] == (right[0] if right else -1)


# ---------------------------------------------------------------- the interface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_LZ_LITERAL\s+0xffffffffu\b", header)
    assert sa.LZ_LITERAL == LIT
    assert "sa_amd_lz_stats" in header
    for field in ("phrases", "literals", "longest", "longest_pos", "unresolved", "hierarchy_steps", "hierarchy_max", "walkers",
                  "walk_steps", "walk_launches", "restarts", "splitter_spacing", "readbacks"):
        assert field in dict(sa.LzStats._fields_), field
        assert re.search(r"\b" + field + r"\b", header[header.index("typedef struct sa_amd_lz_stats"):]), field
    assert ctypes.sizeof(sa.LzStats) == 88
    D = ctypes.CDLL(os.path.join(os.path.dirname(sa.library_path()), "libsuffix_array_amd_diag.so"))
    assert hasattr(D, "sa_amd_test_lz_nsv") and not hasattr(L, "sa_amd_test_lz_nsv")


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(sa.lpf) == ["s", "sa"] and params(sa.lz77) == ["s", "sa"]
    assert inspect.signature(sa.lpf).parameters["sa"].default is None and inspect.signature(sa.lz77).parameters["sa"].default is None
    assert params(sa.last_lz_stats) == [] and params(sa.lz_work_bytes) == ["n"]
    assert params(sa.lpf_device_ptr)[:7] == ["text_ptr", "sa_ptr", "n", "lpf_ptr", "src_ptr", "work_ptr", "work_bytes"]
    assert params(sa.lz77_device_ptr)[:7] == ["text_ptr", "sa_ptr", "n", "phrases_ptr", "capacity", "work_ptr", "work_bytes"]
    assert params(sa.DeviceIndex.lpf) == ["self"] and params(sa.DeviceIndex.lz77) == ["self"]
    assert params(sa.SuffixArray.lpf) == ["self"] and params(sa.SuffixArray.lz77) == ["self"]
    for name in ("lpf", "lz77", "lz77_decode", "lz77_literals", "last_lz_stats", "lz_work_bytes", "lpf_device_ptr", "lz77_device_ptr",
                 "LZ_LITERAL"):
        assert name in sa.__all__


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.zeros(256, dtype=np.uint32)
    p = buf.ctypes.data
    p256 = (p + 255) & ~255
    cnt = ctypes.c_int64(-7)
    c = ctypes.byref(cnt)
    big = 1 << 30
    assert L.sa_amd_lz_work_bytes(-1) == -1
    assert L.sa_amd_lpf(None, -1, None, p, p) == -1                                           # n < 0
    assert L.sa_amd_lpf(None, 4, None, p, p) == -1                                            # null text
    assert L.sa_amd_lz77(p, 4, p, p, -1, c) == -1                                             # negative capacity
    assert L.sa_amd_lz77(p, 4, p, None, 4, c) == -1                                           # null output with room asked for
    assert L.sa_amd_lz77(p, 4, p, p, 4, None) == -1                                           # null count
    assert L.sa_amd_lz77(None, 4, p, p, 4, c) == -1
    assert L.sa_amd_lpf_device(p, p, -1, p, p, p256, big, None) == -1
    assert L.sa_amd_lpf_device(p, None, 4, p, p, p256, big, None) == -1
    assert L.sa_amd_lpf_device(None, p, 4, p, p, p256, big, None) == -1
    assert L.sa_amd_lpf_device(p, p, 4, p, p, None, big, None) == -1
    assert L.sa_amd_lpf_device(p, p, 4, p, p, p256 + 4, big, None) == -1                      # misaligned work
    assert L.sa_amd_lpf_device(p, p, 4, p, p, p256, 16, None) == -1                           # short work
    assert L.sa_amd_lz77_device(p, p, 4, p, -1, c, p256, big, None) == -1
    assert L.sa_amd_lz77_device(p, p, 4, p, 4, None, p256, big, None) == -1
    assert L.sa_amd_lz77_device(p, p, 4, None, 4, c, p256, big, None) == -1
    assert L.sa_amd_lz77_device(p, p, 4, p, 4, c, p256 + 8, big, None) == -1
    assert L.sa_amd_lz77_device(p, p, 4, p, 4, c, p256, 64, None) == -1
    assert L.sa_amd_index_lpf(None, p, p) == -1
    assert L.sa_amd_index_lz77(None, p, 4, c) == -1
    assert cnt.value == -7 and not buf.any()                                                  # nothing written
    st = sa.LzStats()
    L.sa_amd_last_lz_stats(ctypes.byref(st))
    L.sa_amd_last_lz_stats(None)


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 4096, 1 << 20, (1 << 30) + 4097, 2**31 - 1])
def test_work_block(n):
    """the LCP array's block plus three n-entry buffers"""
    L = sa.lib()
    w = L.sa_amd_lz_work_bytes(n)
    assert w % 256 == 0 and w == sa.lz_work_bytes(n)
    assert L.sa_amd_lcp_work_bytes(n) + 12 * n <= w <= L.sa_amd_lcp_work_bytes(n) + 12 * (n + 68) + 256
