"""GPU suite for the Burrows-Wheeler transform and its inverse (kernels/bwt.hpp, host/bwt.hpp): every route against the numpy
definition over the oracle's array, round trips, the resume and restart paths of the walks, the families that beat unhashed
splitters, invalid input, one text above 2^30 bytes and thread safety.  At most two large texts are alive at once."""
import ctypes
import glob
import os
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word
from test_bwt_abi import KNOWN, bwt_definition, invalid_pair, literal_inverse, three_phase_inverse

pytestmark = pytest.mark.gpu

N_ABOVE = (1 << 30) + 4097


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


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


def bwt_on_device(t, arr, offset=0, out_offset=0):
    """sa_amd_bwt_device on hipMalloc'ed buffers; `offset` bytes of misalignment in front of the text, `out_offset` in front of B"""
    n = t.size
    wb = sa.bwt_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), n + 8, wb) as d:
        dT, dS, dB, dW = d.p
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        primary = sa.bwt_device_ptr(dT + offset, dS, n, dB + out_offset, dW, wb)
        out = np.zeros(n, dtype=np.uint8)
        if n:
            assert d.hip.hipMemcpy(out.ctypes.data, dB + out_offset, n, 2) == 0
    return out, primary


def unbwt_on_device(b, primary, offset=0, guard=64):
    """sa_amd_unbwt_device with `guard` canary bytes on both sides of dT_out; returns (status, text, canaries untouched)"""
    n = b.size
    wb = sa.unbwt_work_bytes(n)
    with _Dev(n + 8, n + 2 * guard + 8, wb) as d:
        dB, dO, dW = d.p
        if n:
            assert d.hip.hipMemcpy(dB + offset, b.ctypes.data, n, 1) == 0
        assert d.hip.hipMemset(dO, 0xA5, n + 2 * guard + 8) == 0
        rc = sa.lib().sa_amd_unbwt_device(dB + offset, n, primary, dO + guard + offset, dW, wb, None)
        raw = np.zeros(n + 2 * guard + 8, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
    lo, hi = guard + offset, guard + offset + n
    clean = bool((raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all())
    return rc, raw[lo:hi].copy(), clean, raw


def all_forward_routes(t):
    """bwt with and without sa, bwt_device_ptr at text misalignments 0..3, DeviceIndex.bwt, SuffixArray.bwt: all equal"""
    arr = np.empty(t.size + 1, dtype=np.uint32)
    sa.saca(t, arr)
    b, p = sa.bwt(t, arr)
    routes = [sa.bwt(t)]
    for off in range(4):
        routes.append(bwt_on_device(t, arr, off, (off * 3) & 3))
    ix = sa.DeviceIndex(t, arr)
    routes.append(ix.bwt())
    ix.close()
    ix = sa.DeviceIndex(t)
    routes.append(ix.bwt())
    ix.close()
    routes.append(sa.SuffixArray.unchecked_from_parts(t, arr).bwt())
    for k, (b2, p2) in enumerate(routes):
        assert p2 == p and np.array_equal(b2, b), k
    return arr, b, p


@pytest.mark.parametrize("text,exp_b,exp_p", KNOWN)
def test_known_answers_every_route(text, exp_b, exp_p):
    t = _u8(text)
    _, b, p = all_forward_routes(t)
    assert (b.tobytes(), p) == (exp_b, exp_p)
    assert sa.unbwt(b, p).tobytes() == text
    for off in range(4):
        rc, got, clean, _ = unbwt_on_device(b, p, off)
        assert rc == 0 and clean and got.tobytes() == text


def _both_halves(oracle, t, name):
    exp_b, exp_p = bwt_definition(t, oracle.sais(t))
    _, b, p = all_forward_routes(t)
    assert p == exp_p and np.array_equal(b, exp_b), name
    assert np.array_equal(sa.unbwt(b, p), t), name
    assert np.array_equal(sa.unbwt(exp_b, exp_p), t), name       # the inverse on the NUMPY transform: not only checked against the forward half


def test_adversarial_cases(oracle):
    for name, raw in adversarial_cases().items():
        _both_halves(oracle, _u8(raw), name)


def test_golden_fixtures(oracle):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    files = sorted(glob.glob(os.path.join(here, "*.text")))
    assert files
    for f in files:
        t = np.fromfile(f, dtype=np.uint8)
        arr = np.fromfile(f[:-len(".text")] + ".sa.u32le", dtype="<u4").astype(np.uint32)
        exp_b, exp_p = bwt_definition(t, arr)
        b, p = sa.bwt(t, arr)
        assert p == exp_p and np.array_equal(b, exp_b), f
        _both_halves(oracle, t, f)


@pytest.mark.parametrize("n", [8191, 8192, 8193, 100003])
def test_sizes_around_the_small_text_route(oracle, n):
    rng = np.random.default_rng(n)
    for sigma in (1, 2, 256):
        t = rng.integers(0, sigma, n, dtype=np.uint8)
        _both_halves(oracle, t, (n, sigma))


def test_text_of_one_byte_value_closed_form_array(monkeypatch):
    monkeypatch.delenv("SA_AMD_NO_UNARY_SHORTCUT", raising=False)
    t = np.full((1 << 20) + 3, 0xEE, dtype=np.uint8)
    b, p = sa.bwt(t)
    assert p == t.size and np.array_equal(b, t)
    assert np.array_equal(sa.unbwt(b, p), t)


def test_resume_path_caps(oracle):
    t = corpus.english_corpus(1 << 20, 3)
    n = t.size
    exp_b, exp_p = bwt_definition(t, oracle.sais(t))
    b, p = sa.bwt(t)
    assert p == exp_p and np.array_equal(b, exp_b)
    try:
        for cap in (1, 7, 64):
            sa.unbwt_set_walk_limits(cap, -1)
            assert np.array_equal(sa.unbwt(b, p), t), cap
            st = sa.last_unbwt_stats()
            print("cap", cap, st)
            assert st["walk_launches"] > 1 and st["restarts"] == 0, (cap, st)
            assert st["steps"] <= 2 * (n + 1) + 2 * st["walkers"], (cap, st)      # each row once per walking phase: a resumed walk must not start over
        # the launch limit forced low enough to take the restart
        sa.unbwt_set_walk_limits(64, 2)
        assert np.array_equal(sa.unbwt(b, p), t)
        st = sa.last_unbwt_stats()
        print("restart", st)
        assert st["restarts"] >= 1 and st["splitter_spacing"] < 256, st
        sa.unbwt_set_walk_limits(1, 1)                                           # down to the densest set (no launch limit there)
        assert np.array_equal(sa.unbwt(b, p), t)
        assert sa.last_unbwt_stats()["splitter_spacing"] == 4
    finally:
        sa.unbwt_set_walk_limits(-1, -1)
    assert np.array_equal(sa.unbwt(b, p), t)
    st = sa.last_unbwt_stats()
    assert st["restarts"] == 0 and st["walk_launches"] == 1 and st["steps"] == 2 * (n + 1), st


def _fib_text(n):
    k, w = 1, fibonacci_word(1)
    while len(w) < n:
        k += 1
        w = fibonacci_word(k)
    return np.frombuffer(w[:n], dtype=np.uint8)


@pytest.mark.parametrize("family", ["random", "one_byte", "period2", "fibonacci", "twice", "ramp_rep"])
def test_families_16m_default_cap(family):
    """round trip exact, no restart, and the longest walk within 32 S: the hash really spreads the splitters on these families
    (the longest of m = n / S gaps of mean S is about S ln m; ln m <= 12.5 here, so 32 S leaves e^-19)"""
    n = 1 << 24
    if family == "random":
        t = corpus.uniform(n, 13)
    elif family == "one_byte":
        t = np.full(n, 0x41, dtype=np.uint8)
    elif family == "period2":
        t = np.tile(np.array([1, 2], dtype=np.uint8), n // 2)
    elif family == "fibonacci":
        t = _fib_text(n)
    elif family == "twice":
        h = corpus.uniform(n // 2, 9)
        t = np.concatenate([h, h])
    else:
        t = np.tile(np.arange(256, dtype=np.uint8), n // 256)
    b, p = sa.bwt(t)
    got = sa.unbwt(b, p)
    st = sa.last_unbwt_stats()
    print(family, st)
    assert np.array_equal(got, t)
    assert st["restarts"] == 0, st
    assert st["longest_walk"] <= 32 * st["splitter_spacing"], st
    assert st["steps"] == 2 * (n + 1)


def test_invalid_input(oracle):
    L = sa.lib()
    t = _u8(b"mississippi")
    n = t.size
    arr = oracle.sais(t)
    out = np.zeros(n, dtype=np.uint8)
    prim = ctypes.c_int32(-7)
    for bad_primary in (0, n + 1, -1):
        assert L.sa_amd_unbwt(t.ctypes.data, n, bad_primary, out.ctypes.data) == -1
        with pytest.raises(ValueError):
            sa.unbwt(t, bad_primary)
        rc, _, clean, raw = unbwt_on_device(t, bad_primary)
        assert rc == -1 and clean and (raw == 0xA5).all()
    bad = arr.copy()
    bad[5] = n + 1
    assert L.sa_amd_bwt(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, ctypes.byref(prim)) == -6
    with pytest.raises(IndexError):
        sa.bwt(t, bad)
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]                               # SA[0] != n
    assert L.sa_amd_bwt(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data, ctypes.byref(prim)) == -1
    with pytest.raises(ValueError):
        sa.bwt(t, bad)
    bad = arr.copy()
    bad[7] = 0                                                    # two zero entries
    with pytest.raises(ValueError):
        sa.bwt(t, bad)
    bad = arr.copy()
    bad[int(np.nonzero(arr == 0)[0][0])] = 3                      # no zero entry
    with pytest.raises(ValueError):
        sa.bwt(t, bad)
    assert prim.value == -7
    # the empty text
    assert sa.bwt(b"") [1] == 0 and sa.unbwt(b"", 0).size == 0
    with pytest.raises(ValueError):
        sa.unbwt(b"", 1)
    with pytest.raises(IndexError):
        sa.bwt(b"", np.array([1], dtype=np.uint32))
    # a wrong permutation with the right frame: unspecified bytes, nothing outside B
    perm = arr.copy()
    perm[2], perm[9] = perm[9], perm[2]
    b, p = sa.bwt(t, perm)
    assert b.size == n and 1 <= p <= n
    # "ba", 2: the walk from primary closes after two of three rows
    with pytest.raises(ValueError):
        sa.unbwt(b"ba", 2)
    # a 1 MiB pair whose walk closes early, built by the numpy model; the device form with canaries around dT_out
    b, p = invalid_pair(1 << 20, 7)
    assert L.sa_amd_unbwt(b.ctypes.data, b.size, p, np.zeros(b.size, dtype=np.uint8).ctypes.data) == -1
    with pytest.raises(ValueError):
        sa.unbwt(b, p)
    for off in (0, 1):
        rc, _, clean, raw = unbwt_on_device(b, p, off)
        assert rc == -1 and clean
        assert (raw == 0xA5).all()                                # refused before the writing walk: nothing written at all
    try:
        sa.unbwt_set_walk_limits(3, 2)                            # the same through resumed launches and restarts
        with pytest.raises(ValueError):
            sa.unbwt(b, p)
    finally:
        sa.unbwt_set_walk_limits(-1, -1)
    # short or misaligned work blocks
    with _Dev(n, 4 * (n + 1), n, 4096, sa.unbwt_work_bytes(n)) as d:
        dT, dS, dB, dW, dW2 = d.p
        assert L.sa_amd_bwt_device(dT, dS, n, dB, ctypes.byref(prim), dW, 64, None) == -1
        assert L.sa_amd_bwt_device(dT, dS, n, dB, ctypes.byref(prim), dW + 4, 256, None) == -1
        assert L.sa_amd_bwt_device(dT, dS, n, dT, ctypes.byref(prim), dW, 256, None) == -1       # B may not alias the text
        assert L.sa_amd_unbwt_device(dB, n, 1, dT, dW2, 64, None) == -1
        assert L.sa_amd_unbwt_device(dB, n, 1, dT, dW2 + 4, sa.unbwt_work_bytes(n), None) == -1


def test_model_and_device_agree_on_stats(oracle):
    """the numpy model and the device take the same splitters: walkers, longest walk and launches are equal"""
    t = corpus.english_corpus(20000, 9)
    b, p = bwt_definition(t, oracle.sais(t))
    try:
        for cap, launches in ((5, -1), (None, -1), (2, 3)):
            sa.unbwt_set_walk_limits(-1 if cap is None else cap, launches)
            assert np.array_equal(sa.unbwt(b, p), t)
            st = sa.last_unbwt_stats()
            exp_t, exp = three_phase_inverse(b, p, cap=cap, max_launches=launches)
            assert np.array_equal(exp_t, t)
            for k in exp:
                assert st[k] == exp[k], (cap, launches, k, st, exp)
    finally:
        sa.unbwt_set_walk_limits(-1, -1)


def test_above_2_30_round_trip():
    n = N_ABOVE
    t = corpus.uniform(n, 31)
    ix = sa.DeviceIndex(t)
    assert ix.check_integrity()
    b, p = ix.bwt()
    arr = ix.suffix_array()
    ix.close()
    assert int(arr[p]) == 0 and b[0] == t[n - 1]
    rng = np.random.default_rng(43)
    rows = rng.integers(0, n, 2000)
    src = arr[rows + (rows >= p)].astype(np.int64)
    assert np.array_equal(b[rows], t[src - 1])
    del arr
    sa.lib().sa_amd_release_cache()
    got = sa.unbwt(b, p)
    st = sa.last_unbwt_stats()
    print("above 2^30", st)
    assert st["restarts"] == 0 and st["steps"] == 2 * (n + 1)
    del b
    step = 1 << 26
    for s in range(0, n, step):
        assert np.array_equal(got[s:s + step], t[s:s + step]), s
    del got, t
    sa.lib().sa_amd_release_cache()


def test_thread_safety(oracle):
    texts = [corpus.english_corpus(300000 + 1111 * k, 20 + k) if k % 2 else corpus.dna(200000 + 777 * k, 20 + k) for k in range(4)]
    expected = [bwt_definition(t, oracle.sais(t)) for t in texts]
    errors = []

    def work(k):
        try:
            t = texts[k]
            sa.unbwt_set_walk_limits([-1, 50, 300, -1][k], -1)
            for rep in range(4):
                if (rep + k) % 2:
                    b, p = sa.bwt(t)
                    assert p == expected[k][1] and np.array_equal(b, expected[k][0])
                    assert np.array_equal(sa.unbwt(b, p), t)
                else:
                    assert np.array_equal(sa.unbwt(*expected[k]), t)
                    b, p = sa.bwt(t)
                    assert p == expected[k][1] and np.array_equal(b, expected[k][0])
                st = sa.last_unbwt_stats()
                assert st["steps"] == 2 * (t.size + 1) and st["restarts"] == 0
        except BaseException as e:      # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_profile_classes_report_bwt_kernels():
    L = sa.lib()
    names = []
    while True:
        nm = L.sa_amd_profile_kernel_name(len(names)).decode()
        if not nm:
            break
        names.append(nm)
    assert len(names) <= 32
    t = corpus.english_corpus(1 << 20, 8)
    L.sa_amd_profile_begin()
    b, p = sa.bwt(t)
    assert np.array_equal(sa.unbwt(b, p), t)
    cap = 32
    ms, launches, units = (ctypes.c_double * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
    cnt = L.sa_amd_profile_end(ms, launches, units, cap)
    got = {names[i]: launches[i] for i in range(cnt)}
    for k in ("k_bwt_gather", "k_unbwt_walk", "k_unbwt_rank", "k_unbwt_write"):
        assert got[k] > 0, (k, got)
