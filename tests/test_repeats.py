"""GPU suite for repeat finding: every route (host pointers with and without the array, device pointers, DeviceIndex, SuffixArray)
against the numpy definitions of test_repeats_abi.py over the oracle's suffix array and Kasai's LCP array."""
import ctypes
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, adversarial_cases, fibonacci_word
from test_lcp import _Dev, _u8, kasai, work_bound
from test_repeats_abi import (check_invariants, keep_first_definition, repeat_lengths_definition, spans_definition,
                              stats_definition)

pytestmark = pytest.mark.gpu

SMALL_MAX = 8192
N_ABOVE = (1 << 30) + 4097
CANARY = 0xA5


def expected(oracle, t, arr=None):
    if arr is None:
        arr = oracle.sais(t)
    lcp = kasai(oracle, t, arr)
    return arr, lcp, repeat_lengths_definition(t, arr, lcp)


def expected_spans(t, arr, lcp, lr, k, keep_first):
    return keep_first_definition(t, arr, lcp, k) if keep_first else spans_definition(lr, k)


def check_stats(t, lcp, lr, spans, flagged, got=None):
    got = sa.last_repeat_stats() if got is None else got
    exp = stats_definition(t, lcp, lr, spans, flagged)
    for key, val in exp.items():
        assert got[key] == val, (key, got, exp)
    assert got["readbacks"] >= 1


def lengths_on_device(t, arr, offset=0):
    """sa_amd_repeat_lengths_device on hipMalloc'ed buffers, `offset` bytes of misalignment in front of the text and 256 canary
    bytes on either side of dLR"""
    n = t.size
    wb = sa.repeats_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), 4 * n + 512, wb) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 4 * n + 512) == 0
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        sa.repeat_lengths_device_ptr(dT + offset, dS, n, dO + 256, dW, wb)
        raw = np.zeros(4 * n + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
    assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 4 * n:] == CANARY)
    return raw[256:256 + 4 * n].view(np.uint32).copy()


def spans_on_device(t, arr, k, mode, capacity, offset=0):
    """sa_amd_repeat_spans_device likewise; returns (count, the `capacity` pairs of the buffer as they came back)"""
    n = t.size
    wb = sa.repeats_work_bytes(n)
    with _Dev(n + 8, 4 * (n + 1), 8 * capacity + 512, wb) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * capacity + 512) == 0
        if n:
            assert d.hip.hipMemcpy(dT + offset, t.ctypes.data, n, 1) == 0
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        assert d.hip.hipMemcpy(dS, a.ctypes.data, 4 * (n + 1), 1) == 0
        count = sa.repeat_spans_device_ptr(dT + offset, dS, n, k, mode, dO + 256, capacity, dW, wb)
        raw = np.zeros(8 * capacity + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
    assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 8 * capacity:] == CANARY)
    body = raw[256:256 + 8 * capacity]
    wrote = min(count, capacity)
    assert np.all(body[8 * wrote:] == CANARY)                         # nothing behind the spans that exist
    return count, body[:8 * wrote].view(np.uint32).reshape(-1, 2).astype(np.int64)


def check_all_routes(oracle, t, ks, name="", offsets=(0,), arr=None):
    n = t.size
    arr, lcp, lr = expected(oracle, t, arr)
    empty = np.zeros((0, 2), dtype=np.int64)
    assert np.array_equal(sa.repeat_lengths(t), lr), name
    check_stats(t, lcp, lr, empty, np.zeros(0))
    assert np.array_equal(sa.repeat_lengths(t, arr), lr), name
    for off in offsets:
        assert np.array_equal(lengths_on_device(t, arr, off), lr), (name, off)
    ix = sa.DeviceIndex(t, arr)
    s = sa.SuffixArray.unchecked_from_parts(t, arr)
    assert np.array_equal(ix.repeat_lengths(), lr), name
    assert np.array_equal(s.repeat_lengths(), lr), name
    for k in ks:
        both = []
        for keep_first in (False, True):
            exp, flagged = expected_spans(t, arr, lcp, lr, k, keep_first)
            both.append(exp)
            got = sa.repeat_spans(t, k, keep_first)
            assert got.dtype == np.uint32 and got.shape == exp.shape and np.array_equal(got, exp), (name, k, keep_first)
            check_stats(t, lcp, lr, exp, flagged)
            assert np.array_equal(sa.repeat_spans(t, k, keep_first, sa=arr), exp), (name, k, keep_first)
            assert np.array_equal(ix.repeat_spans(k, keep_first), exp), (name, k, keep_first)
            check_stats(t, lcp, lr, exp, flagged)
            assert np.array_equal(s.repeat_spans(k, keep_first), exp), (name, k, keep_first)
            cap = sa.repeat_spans_bound(n, k)
            for off in offsets:
                count, dev = spans_on_device(t, arr, k, int(keep_first), cap, off)
                assert count == exp.shape[0] and np.array_equal(dev, exp), (name, k, keep_first, off)
        check_invariants(t, lr, k, both[0], both[1])
    ix.close()


def _ks(n):
    return sorted({1, 2, 50, max(n, 1), n + 1})


def test_known_answers():
    t = _u8(b"banana")
    assert sa.repeat_lengths(t).tolist() == [0, 3, 2, 3, 2, 1]       # (see test_repeats_abi.test_known_answers for LR[3])
    st = sa.last_repeat_stats()
    assert st["longest"] == 3 and st["longest_pos"] == 1 and st["lcp_sum"] == 6 and st["distinct_substrings"] == 15
    assert st["spans"] == 0 and st["covered_bytes"] == 0 and st["flagged"] == 0
    assert sa.repeat_spans(t, 2).tolist() == [[1, 6]]
    assert sa.repeat_spans(t, 2, keep_first=True).tolist() == [[3, 6]]
    t = _u8(b"mississippi")
    assert sa.repeat_lengths(t).tolist() == [0, 4, 3, 2, 4, 3, 2, 1, 1, 1, 1]
    assert sa.repeat_spans(t, 2).tolist() == [[1, 8]] and sa.repeat_spans(t, 2, True).tolist() == [[4, 8]]
    assert sa.repeat_spans(t, 1, True).tolist() == [[3, 8], [9, 11]]
    assert sa.repeat_spans(t, 5).shape == (0, 2)


def test_tiny_texts(oracle):
    assert sa.repeat_lengths(b"").shape == (0,)
    st = sa.last_repeat_stats()
    assert all(st[key] == 0 for key in st if key not in ("longest_pos", "readbacks")) and st["longest_pos"] == -1
    assert sa.repeat_spans(b"", 1).shape == (0, 2) and sa.repeat_spans(b"", 1, True).shape == (0, 2)
    assert sa.repeat_lengths(b"x").tolist() == [0]
    for b in (b"", b"a", b"aa", b"ab", b"ba"):
        check_all_routes(oracle, _u8(b), _ks(len(b)), b, offsets=(0, 1, 2, 3))


def test_adversarial_cases_all_routes(oracle):
    for name, b in adversarial_cases().items():
        t = _u8(b)
        check_all_routes(oracle, t, _ks(t.size), name, offsets=(0, 1, 2, 3) if t.size <= 600 else (0, 3))


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
        check_all_routes(oracle, t, _ks(t.size), name, arr=arr)


@pytest.mark.parametrize("n", [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 2047, 2048, 2049, 100003])
def test_sizes_around_the_small_path_and_the_tile(oracle, n):
    t = corpus.english_corpus(n, 5)
    check_all_routes(oracle, t, (1, 2, 50, n), n, offsets=(0, 1))
    t = np.random.default_rng(n).integers(0, 2, n, dtype=np.uint8)
    check_all_routes(oracle, t, (1, 7, 13), n)


@pytest.mark.parametrize("knob", ["SA_AMD_BINNED_ISA_ALWAYS", "SA_AMD_NO_BINNED_ISA"])
def test_binned_scatter_forced(oracle, monkeypatch, knob):
    monkeypatch.setenv(knob, "1")
    for n in (1, 2, 700, 5000, 300000):
        t = corpus.english_corpus(n, 11)
        check_all_routes(oracle, t, (1, 2, 50), (knob, n))
    monkeypatch.setenv("SA_AMD_SCATTER_LEVELS", "2")
    t = corpus.dna(200000, 4)
    check_all_routes(oracle, t, (2, 50), (knob, "two levels"))


@pytest.mark.parametrize("n", [(1 << 25) - 3, (1 << 25) + 5])
def test_sizes_around_the_binned_threshold(oracle, n):
    t = corpus.english_corpus(n, 6)
    arr = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, arr)
    arr, lcp, lr = expected(oracle, t, arr)
    assert np.array_equal(sa.repeat_lengths(t, arr), lr)
    assert np.array_equal(lengths_on_device(t, arr, 1), lr)           # the caller's dLR between canaries, on the route n itself selects
    cap = sa.repeat_spans_bound(n, 50)
    for keep_first in (False, True):
        exp, flagged = expected_spans(t, arr, lcp, lr, 50, keep_first)
        assert np.array_equal(sa.repeat_spans(t, 50, keep_first, sa=arr), exp)
        check_stats(t, lcp, lr, exp, flagged)
        count, dev = spans_on_device(t, arr, 50, int(keep_first), cap, 3)
        assert count == exp.shape[0] and np.array_equal(dev, exp), keep_first
        check_stats(t, lcp, lr, exp, flagged)


def _plant(n, seed, pieces=200):
    rng = np.random.default_rng(seed)
    t = corpus.uniform(n, seed).copy()
    placed = []
    slot = n // (2 * pieces)
    for j in range(pieces):
        length = int(rng.integers(64, 4097))
        src = j * slot + int(rng.integers(0, slot - 4097))
        dst = n // 2 + j * slot + int(rng.integers(0, slot - 4097))
        t[dst:dst + length] = t[src:src + length]
        placed.append((src, dst, length))
    return t, placed


def _inside(spans, a, b):
    i = int(np.searchsorted(spans[:, 0], a, side="right")) - 1
    return i >= 0 and spans[i, 0] <= a and b <= spans[i, 1]


def test_planted_copies(oracle):
    n = 1 << 22
    t, placed = _plant(n, 17)
    arr = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, arr)
    arr, lcp, lr = expected(oracle, t, arr)
    exp_all, fl_all = spans_definition(lr, 32)
    got_all = sa.repeat_spans(t, 32).astype(np.int64)
    st_all = sa.last_repeat_stats()
    assert np.array_equal(got_all, exp_all)
    check_stats(t, lcp, lr, exp_all, fl_all, st_all)
    exp_kf, fl_kf = keep_first_definition(t, arr, lcp, 32)
    got_kf = sa.repeat_spans(t, 32, keep_first=True).astype(np.int64)
    assert np.array_equal(got_kf, exp_kf)
    check_stats(t, lcp, lr, exp_kf, fl_kf)
    for src, dst, length in placed:
        assert _inside(got_all, src, src + length) and _inside(got_all, dst, dst + length), (src, dst, length)
        assert _inside(got_kf, dst, dst + length), (src, dst, length)
        assert not _inside(got_kf, src, src + 1), (src, dst, length)
    print("planted bytes", 2 * sum(p[2] for p in placed), "covered", st_all["covered_bytes"], "spans", st_all["spans"])


def test_english_corpus_16m_stats_exact(oracle):
    n = 16 << 20
    t = corpus.english_corpus(n, 3)
    arr = np.empty(n + 1, dtype=np.uint32)
    sa.saca(t, arr)
    arr, lcp, lr = expected(oracle, t, arr)
    assert np.array_equal(sa.repeat_lengths(t), lr)
    for keep_first in (False, True):
        exp, flagged = expected_spans(t, arr, lcp, lr, 50, keep_first)
        got = sa.repeat_spans(t, 50, keep_first)
        assert np.array_equal(got, exp), keep_first
        check_stats(t, lcp, lr, exp, flagged)
        assert exp.shape[0] > 0


def _fib_text(n):
    k, w = 1, fibonacci_word(1)
    while len(w) < n:
        k += 1
        w = fibonacci_word(k)
    return np.frombuffer(w[:n], dtype=np.uint8)


@pytest.mark.parametrize("family", ["one_byte", "period2", "fibonacci", "twice"])
def test_long_lcp_families_16m(oracle, family):
    n = 1 << 24
    k = 50
    if family == "one_byte":
        t = np.full(n, 0x41, dtype=np.uint8)
        arr = np.arange(n, -1, -1, dtype=np.uint32)
    else:
        if family == "period2":
            t = np.tile(np.array([1, 2], dtype=np.uint8), n // 2)
        elif family == "twice":
            h = corpus.uniform(n // 2, 9)
            t = np.concatenate([h, h])
        else:
            t = _fib_text(n)
        arr = np.empty(n + 1, dtype=np.uint32)
        sa.saca(t, arr)
    got_all = sa.repeat_spans(t, k, sa=arr)
    assert sa.last_lcp_stats()["compared_bytes"] <= work_bound(n), family
    got_kf = sa.repeat_spans(t, k, keep_first=True, sa=arr)
    assert sa.last_lcp_stats()["compared_bytes"] <= work_bound(n), family
    st = sa.last_repeat_stats()
    got_lr = sa.repeat_lengths(t, arr)
    if family == "one_byte":                                          # closed forms: LR = [n-1, n-1, n-2, .., 1]
        assert got_all.tolist() == [[0, n]] and got_kf.tolist() == [[1, n]]
        assert got_lr[0] == n - 1 and np.array_equal(got_lr[1:], np.arange(n - 1, 0, -1, dtype=np.uint32))
        assert st["flagged"] == n - k and st["longest"] == n - 1 and st["longest_pos"] == 0 and st["lcp_sum"] == n * (n - 1) // 2
    elif family == "period2":                                         # LR = [n-2, n-3, n-2, n-3, .., 1]; the first k-windows at 0 and 1
        assert got_all.tolist() == [[0, n]] and got_kf.tolist() == [[2, n]]
        assert got_lr[0] == n - 2 and got_lr[1] == n - 3 and np.array_equal(got_lr[2:], np.arange(n - 2, 0, -1, dtype=np.uint32))
        assert st["longest"] == n - 2 and st["longest_pos"] == 0
    elif family == "twice":
        assert got_all.tolist() == [[0, n]] and got_kf.tolist() == [[n // 2, n]]
        assert st["longest"] == n // 2 and st["longest_pos"] == 0
    arr, lcp, lr = expected(oracle, t, arr)
    assert np.array_equal(got_lr, lr), family
    exp_all, _ = spans_definition(lr, k)
    exp_kf, fl_kf = keep_first_definition(t, arr, lcp, k)
    assert np.array_equal(got_all, exp_all) and np.array_equal(got_kf, exp_kf), family
    assert exp_all.tolist() == [[0, n]], family                      # one span
    check_stats(t, lcp, lr, exp_kf, fl_kf, st)


_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import suffix_array_amd as sa
n = {n}
t = np.full(n, 0x41, dtype=np.uint8)
arr = np.arange(n, -1, -1, dtype=np.uint32)
got = sa.repeat_spans(t, {k}, keep_first=True, sa=arr)
print(json.dumps({{"spans": got.tolist(), "stats": sa.last_repeat_stats(), "lcp": sa.last_lcp_stats()}}))
"""


def test_keep_first_run_over_the_whole_array_under_a_time_limit():
    """a^n is ONE slot run: the segmented minimum has to cross every tile.  The GPU step runs in a child process under a time
    limit of its own, so a route that walks a run member by member fails here instead of hanging the suite."""
    import json
    import subprocess
    import sys
    n, k = 1 << 24, 50
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, n=n, k=k)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["spans"] == [[1, n]]
    st = res["stats"]
    assert st["spans"] == 1 and st["covered_bytes"] == n - 1 and st["flagged"] == n - k
    assert st["longest"] == n - 1 and st["longest_pos"] == 0 and st["lcp_sum"] == n * (n - 1) // 2
    assert res["lcp"]["compared_bytes"] <= work_bound(n)


def test_truncation(oracle):
    t = corpus.english_corpus(300000, 12)
    arr, lcp, lr = expected(oracle, t)
    for mode in (0, 1):
        exp, flagged = expected_spans(t, arr, lcp, lr, 20, bool(mode))
        total = exp.shape[0]
        assert total > 8
        for cap in (0, 1, 7, total - 1, total, total + 5):
            count, dev = spans_on_device(t, arr, 20, mode, cap)
            assert count == total and np.array_equal(dev, exp[:cap]), (mode, cap)
            check_stats(t, lcp, lr, exp, flagged)
        out = np.full((5, 2), 0xEEEEEEEE, dtype=np.uint32)
        cnt = ctypes.c_int64(0)
        assert sa.lib().sa_amd_repeat_spans(t.ctypes.data, t.size, None, 20, mode, out.ctypes.data, 3, ctypes.byref(cnt)) == 0
        assert cnt.value == total and np.array_equal(out[:3], exp[:3]) and np.all(out[3:] == 0xEEEEEEEE)
        check_stats(t, lcp, lr, exp, flagged)


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
    assert L.sa_amd_repeat_lengths(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data) == -6
    assert L.sa_amd_repeat_spans(t.ctypes.data, n, bad.ctypes.data, 2, 0, out.ctypes.data, n, c) == -6
    with pytest.raises(IndexError):
        sa.repeat_lengths(t, bad)
    with pytest.raises(IndexError):
        sa.repeat_spans(t, 2, sa=bad)
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]
    assert L.sa_amd_repeat_lengths(t.ctypes.data, n, bad.ctypes.data, out.ctypes.data) == -1
    assert L.sa_amd_repeat_spans(t.ctypes.data, n, bad.ctypes.data, 2, 1, out.ctypes.data, n, c) == -1
    with pytest.raises(ValueError):
        sa.repeat_spans(t, 2, keep_first=True, sa=bad)
    assert L.sa_amd_repeat_spans(t.ctypes.data, n, arr.ctypes.data, 0, 0, out.ctypes.data, n, c) == -1       # min_len 0
    assert L.sa_amd_repeat_spans(t.ctypes.data, n, arr.ctypes.data, 2, 2, out.ctypes.data, n, c) == -1       # bad mode
    assert L.sa_amd_repeat_spans(t.ctypes.data, n, arr.ctypes.data, 2, 0, out.ctypes.data, -1, c) == -1      # negative capacity
    assert cnt.value == -5 and np.all(out == 0x77777777)                                                     # nothing written
    zero = np.zeros(1, dtype=np.uint32)
    assert L.sa_amd_repeat_lengths(None, 0, np.array([1], dtype=np.uint32).ctypes.data, zero.ctypes.data) == -6
    assert L.sa_amd_repeat_spans(None, 0, np.array([0], dtype=np.uint32).ctypes.data, 1, 0, None, 0, c) == 0 and cnt.value == 0
    wb = sa.repeats_work_bytes(n)
    with _Dev(n, 4 * (n + 1), 8 * n + 512, wb + 256) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 8 * n + 512) == 0
        assert d.hip.hipMemcpy(dS, arr.ctypes.data, 4 * (n + 1), 1) == 0
        assert d.hip.hipMemcpy(dT, t.ctypes.data, n, 1) == 0
        cnt.value = -5
        assert L.sa_amd_repeat_lengths_device(dT, dS, n, dO, dW, 64, None) == -1                            # short work block
        assert L.sa_amd_repeat_lengths_device(dT, dS, n, dO, dW + 4, wb, None) == -1                        # misaligned work block
        assert L.sa_amd_repeat_spans_device(dT, dS, n, 2, 0, dO, n, c, dW + 128, wb, None) == -1
        assert L.sa_amd_repeat_spans_device(dT, dS, n, 0, 0, dO, n, c, dW, wb, None) == -1
        assert L.sa_amd_repeat_spans_device(dT, dS, n, 2, 5, dO, n, c, dW, wb, None) == -1
        raw = np.zeros(8 * n + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
        assert np.all(raw == CANARY) and cnt.value == -5
        assert L.sa_amd_repeat_spans_device(dT, dS, n, 2, 0, dO, n, c, dW, wb, None) == 0 and cnt.value == 1


def test_wrong_permutation_stays_in_bounds():
    """unspecified answers, but the outputs' canaries hold and every span lies inside the text"""
    rng = np.random.default_rng(77)
    n = 50000
    t = corpus.english_corpus(n, 2)
    arr = np.empty(n + 1, dtype=np.uint32)
    arr[0] = n
    arr[1:] = rng.integers(0, n, n)                                   # in range, SA[0] = n, far from a permutation
    lengths_on_device(t, arr, 1)
    for mode in (0, 1):
        count, dev = spans_on_device(t, arr, 3, mode, sa.repeat_spans_bound(n, 3))
        assert np.all(dev[:, 0] < dev[:, 1]) and np.all(dev[:, 1] <= n)


def test_profile_classes_report_repeat_kernels():
    L = sa.lib()
    names = []
    while True:
        nm = L.sa_amd_profile_kernel_name(len(names)).decode()
        if not nm:
            break
        names.append(nm)
    assert len(names) <= 32 and names[-2:] == ["k_rep_lr", "k_rep_spans"]
    assert names.index("k_bwt_gather") == 23 and names.index("k_lcp_phi") == 18      # the earlier classes keep their indices
    t = corpus.english_corpus(1 << 20, 8)
    L.sa_amd_profile_begin()
    sa.repeat_spans(t, 50, keep_first=True)
    cap = 32
    ms, launches, units = (ctypes.c_double * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
    cnt = L.sa_amd_profile_end(ms, launches, units, cap)
    got = {names[i]: launches[i] for i in range(cnt)}
    for key in ("k_lcp_phi", "k_lcp_irreducible", "k_lcp_scan", "k_rep_lr", "k_rep_spans"):
        assert got[key] > 0, (key, got)
    assert got["k_lcp_gather"] == 0
    st = sa.last_lcp_stats()
    assert st["irreducible"] > 0 and st["readbacks"] >= 3


def test_top_of_range_planted_copies_sampled():
    n = N_ABOVE
    t, placed = _plant(n, 23, pieces=64)
    ix = sa.DeviceIndex(t)                                            # the array is built on the device, once, and stays there
    got_all = ix.repeat_spans(32).astype(np.int64)
    st_all = sa.last_repeat_stats()
    got_kf = ix.repeat_spans(32, keep_first=True).astype(np.int64)
    st_kf = sa.last_repeat_stats()
    ix.close()
    planted = sum(p[2] for p in placed)
    for sp, st in ((got_all, st_all), (got_kf, st_kf)):
        assert st["spans"] == sp.shape[0] and st["covered_bytes"] == int(np.sum(sp[:, 1] - sp[:, 0]))
        assert np.all(sp[:, 1] - sp[:, 0] >= 32) and np.all(sp[1:, 0] > sp[:-1, 1]) and sp[-1, 1] <= n
    for src, dst, length in placed:
        assert _inside(got_all, src, src + length) and _inside(got_all, dst, dst + length), (src, dst, length)
        assert _inside(got_kf, dst, dst + length) and not _inside(got_kf, src, src + 1), (src, dst, length)
    # every span is a real repeat: its first 32 bytes occur again at the planted partner's offset
    starts = {src: dst for src, dst, _ in placed}
    starts.update({dst: src for src, dst, _ in placed})
    for a, b in got_all:
        near = min(starts, key=lambda x: abs(x - a))
        other = starts[near] + (a - near)
        assert np.array_equal(t[a:a + 32], t[other:other + 32]), (a, b)
    assert got_all.shape[0] <= 2 * len(placed) and got_kf.shape[0] <= len(placed)
    assert 2 * planted <= st_all["covered_bytes"] <= 2 * planted + 2 * 64 * len(placed)
    assert st_all["longest"] >= max(p[2] for p in placed)
    rng = np.random.default_rng(5)                                    # sampled windows elsewhere are not covered
    for x in rng.integers(0, n - 1, 2000):
        if not any(lo - 64 <= x < lo + ln + 64 for s_, d_, ln in placed for lo in (s_, d_)):
            assert not _inside(got_all, int(x), int(x) + 1), x
    del t
    sa.lib().sa_amd_release_cache()


def test_thread_safety(oracle):
    texts = [corpus.english_corpus(200000 + 1000 * j, 20 + j) for j in range(4)]
    exp = []
    for t in texts:
        arr, lcp, lr = expected(oracle, t)
        sp, fl = keep_first_definition(t, arr, lcp, 30)
        exp.append((lcp, lr, sp, fl))
    errors = []

    def work(j):
        try:
            for _ in range(3):
                got = sa.repeat_spans(texts[j], 30, keep_first=True)
                st = sa.last_repeat_stats()
                assert np.array_equal(got, exp[j][2])
                check_stats(texts[j], exp[j][0], exp[j][1], exp[j][2], exp[j][3], st)
                assert np.array_equal(sa.repeat_lengths(texts[j]), exp[j][1])
                assert sa.last_repeat_stats()["spans"] == 0
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
