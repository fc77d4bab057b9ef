"""CPU suite for repeat finding: the definitions of include/suffix_array_amd.h restated in numpy (longest-repeat array, spans of
both modes) and checked against literal brute force, their invariants, known answers, the exports, the Python surface and the
argument checks that answer without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases
from test_lcp_abi import _kasai

EXPORTS = ("sa_amd_repeats_work_bytes", "sa_amd_repeat_spans_bound", "sa_amd_repeat_lengths_device", "sa_amd_repeat_spans_device",
           "sa_amd_repeat_lengths", "sa_amd_repeat_spans", "sa_amd_index_repeat_lengths", "sa_amd_index_repeat_spans",
           "sa_amd_last_repeat_stats")


# ---------------------------------------------------------------- the definitions ----

def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def repeat_lengths_definition(t, arr, lcp):
    """LR[SA[i]] = max(LCP[i], LCP[i + 1]) for 1 <= i <= n, LCP[n + 1] read as 0"""
    n = t.size
    ext = np.concatenate([np.asarray(lcp, dtype=np.int64), [0]])
    lr = np.zeros(n, dtype=np.int64)
    lr[np.asarray(arr[1:], dtype=np.int64)] = np.maximum(ext[1:n + 1], ext[2:n + 2])
    return lr


def intervals(covered):
    """maximal runs of True as an (m, 2) array of [start, end)"""
    c = np.concatenate([[0], np.asarray(covered, dtype=np.int8), [0]])
    d = np.diff(c)
    return np.stack([np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]], axis=1).astype(np.int64)


def _union(starts, lengths, n):
    """the positions inside some [starts[j], starts[j] + lengths[j])"""
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, starts, 1)
    np.add.at(diff, starts + lengths, -1)
    return np.cumsum(diff[:n]) > 0


def spans_definition(lr, k):
    """mode ALL: the union of [p, p + LR[p]) over the p with LR[p] >= k.  Returns (spans, flagged positions)."""
    lr = np.asarray(lr, dtype=np.int64)
    p = np.nonzero(lr >= k)[0]
    return intervals(_union(p, lr[p], lr.size)), p


def keep_first_definition(t, arr, lcp, k):
    """mode KEEP_FIRST by the slot-run rule: in every maximal run of slots [a, b] with LCP[a + 1 .. b] >= k all members but the
    one with the smallest SA value are flagged.  Returns (spans, flagged positions ascending)."""
    n = t.size
    if n == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
    s = np.asarray(arr[1:], dtype=np.int64)                          # slots 1 .. n
    head = np.asarray(lcp[1:], dtype=np.int64) < k                    # slot i starts a run (LCP[1] = 0: always)
    first = np.nonzero(head)[0]
    run_min = np.minimum.reduceat(s, first)
    flagged = np.sort(s[s != run_min[np.cumsum(head) - 1]])
    return intervals(_union(flagged, np.full(flagged.size, k, dtype=np.int64), n)), flagged


def stats_definition(t, lcp, lr, spans, flagged):
    n = t.size
    longest = int(np.max(lcp)) if n else 0
    total = int(np.sum(np.asarray(lcp, dtype=np.int64)))
    return {"longest": longest, "longest_pos": int(np.nonzero(lr == longest)[0][0]) if longest else -1, "lcp_sum": total,
            "distinct_substrings": n * (n + 1) // 2 - total, "spans": int(spans.shape[0]),
            "covered_bytes": int(np.sum(spans[:, 1] - spans[:, 0])), "flagged": int(flagged.size)}


# ---------------------------------------------------------------- literal brute force ----

def brute_lr(t):
    """O(n^2): for every distance d the match lengths of (p, p + d), the longest match of every position over all partners"""
    n = t.size
    lr = np.zeros(n, dtype=np.int64)
    for d in range(1, n):
        m = n - d
        eq = t[:m] == t[d:]
        stop = np.where(~eq, np.arange(m), m)                         # the next mismatch at or behind p
        h = np.minimum.accumulate(stop[::-1])[::-1] - np.arange(m)
        lr[:m] = np.maximum(lr[:m], h)
        lr[d:] = np.maximum(lr[d:], h)
    return lr


def brute_keep_first(t, k):
    """the earlier-window rule, literally: p is flagged iff T[p .. p + k) was seen at some q < p"""
    seen, flagged = set(), []
    raw = t.tobytes()
    for p in range(0, t.size - k + 1):
        w = raw[p:p + k]
        if w in seen:
            flagged.append(p)
        seen.add(w)
    flagged = np.asarray(flagged, dtype=np.int64)
    return intervals(_union(flagged, np.full(flagged.size, k, dtype=np.int64), t.size)), flagged


def brute_all(t, k):
    """every byte inside some occurrence of a substring of length >= k that occurs at least twice"""
    lr = brute_lr(t)
    covered = np.zeros(t.size, dtype=bool)
    for p in range(t.size):
        if lr[p] >= k:
            covered[p:p + lr[p]] = True
    return intervals(covered)


def check_invariants(t, lr, k, spans_all, spans_kf):
    n = t.size
    reach = np.arange(n) + lr
    assert np.all(reach <= n)
    assert np.all(np.diff(reach) >= 0)                                # LR[p] >= LR[p - 1] - 1
    bound = (n + 1) // (k + 1)
    for sp in (spans_all, spans_kf):
        assert sp.shape[0] <= bound
        assert np.all(sp[:, 1] - sp[:, 0] >= k)
        assert np.all(sp[1:, 0] > sp[:-1, 1])                         # ascending, disjoint, not adjacent
        assert sp.size == 0 or (sp[0, 0] >= 0 and sp[-1, 1] <= n)
    ca, ck = np.zeros(n + 1, dtype=bool), np.zeros(n + 1, dtype=bool)
    for a, b in spans_all:
        ca[a:b] = True
    for a, b in spans_kf:
        ck[a:b] = True
    assert not np.any(ck & ~ca)                                       # KEEP_FIRST inside ALL


def _ks(n):
    return sorted({1, 2, 3, 7, 50, max(n, 1), n + 1})


# ---------------------------------------------------------------- tests of the definitions ----

def test_definitions_match_brute_force_on_adversarial_cases(oracle):
    for name, b in adversarial_cases().items():
        if len(b) > 600:
            continue
        t = _u8(b)
        arr = oracle.sais(t)
        lcp = _kasai(oracle, t, arr)
        lr = repeat_lengths_definition(t, arr, lcp)
        assert np.array_equal(lr, brute_lr(t)), name
        for k in _ks(t.size):
            sp_all, fl_all = spans_definition(lr, k)
            sp_kf, fl_kf = keep_first_definition(t, arr, lcp, k)
            assert np.array_equal(sp_all, brute_all(t, k)), (name, k)
            b_sp, b_fl = brute_keep_first(t, k)
            assert np.array_equal(fl_kf, b_fl), (name, k)
            assert np.array_equal(sp_kf, b_sp), (name, k)
            check_invariants(t, lr, k, sp_all, sp_kf)


def test_definitions_match_brute_force_on_random_texts(oracle):
    rng = np.random.default_rng(20261)
    for trial in range(400):
        sigma = int(rng.integers(1, 5))
        n = int(rng.integers(0, 41))
        t = rng.integers(0, sigma, n, dtype=np.uint8) + 97
        arr = oracle.sais(t)
        lcp = _kasai(oracle, t, arr)
        lr = repeat_lengths_definition(t, arr, lcp)
        assert np.array_equal(lr, brute_lr(t)), trial
        subs = {t.tobytes()[i:j] for i in range(n) for j in range(i + 1, n + 1)}
        assert n * (n + 1) // 2 - int(lcp.sum()) == len(subs), trial
        for k in (1, 2, 3, 5, n, n + 1):
            if k < 1:
                continue
            sp_all, _ = spans_definition(lr, k)
            sp_kf, fl_kf = keep_first_definition(t, arr, lcp, k)
            assert np.array_equal(sp_all, brute_all(t, k)), (trial, k)
            b_sp, b_fl = brute_keep_first(t, k)
            assert np.array_equal(fl_kf, b_fl) and np.array_equal(sp_kf, b_sp), (trial, k)
            check_invariants(t, lr, k, sp_all, sp_kf)


def test_definitions_hold_their_invariants_on_larger_texts(oracle):
    for name, b in adversarial_cases().items():
        if len(b) <= 600:
            continue
        t = _u8(b)
        arr = oracle.sais(t)
        lcp = _kasai(oracle, t, arr)
        lr = repeat_lengths_definition(t, arr, lcp)
        for k in (1, 2, 50, t.size):
            sp_all, _ = spans_definition(lr, k)
            sp_kf, _ = keep_first_definition(t, arr, lcp, k)
            check_invariants(t, lr, k, sp_all, sp_kf)


def _answers(oracle, b, k):
    t = _u8(b)
    arr = oracle.sais(t)
    lcp = _kasai(oracle, t, arr)
    lr = repeat_lengths_definition(t, arr, lcp)
    sp_all, fl = spans_definition(lr, k)
    sp_kf, _ = keep_first_definition(t, arr, lcp, k)
    return lr.tolist(), sp_all.tolist(), sp_kf.tolist(), stats_definition(t, lcp, lr, sp_all, fl)


def test_known_answers(oracle):
    """"banana", "mississippi" and a^n written out.  The feature request lists LR("banana") as [0, 3, 2, 1, 2, 1]; its own
    definition gives LR[3] = 3 ("ana" at 3 also starts at 1; slot rule: SA[2] = 3, max(LCP[2], LCP[3]) = max(1, 3)), and so does
    the brute force above, so [0, 3, 2, 3, 2, 1] is what is asserted.  longest_pos and both span lists are as requested."""
    lr, sp_all, sp_kf, st = _answers(oracle, b"banana", 2)
    assert lr == [0, 3, 2, 3, 2, 1] == brute_lr(_u8(b"banana")).tolist()
    assert sp_all == [[1, 6]] and sp_kf == [[3, 6]]
    assert st["longest"] == 3 and st["longest_pos"] == 1 and st["lcp_sum"] == 6 and st["distinct_substrings"] == 15
    assert st["spans"] == 1 and st["covered_bytes"] == 5 and st["flagged"] == 4

    lr, sp_all, sp_kf, st = _answers(oracle, b"mississippi", 2)
    assert lr == [0, 4, 3, 2, 4, 3, 2, 1, 1, 1, 1]
    assert sp_all == [[1, 8]] and sp_kf == [[4, 8]]
    assert st["longest"] == 4 and st["longest_pos"] == 1 and st["lcp_sum"] == 13 and st["distinct_substrings"] == 53
    assert _answers(oracle, b"mississippi", 4)[1:3] == ([[1, 8]], [[4, 8]])          # "issi" at 1 and 4
    assert _answers(oracle, b"mississippi", 5)[1:3] == ([], [])
    assert _answers(oracle, b"mississippi", 1)[2] == [[3, 8], [9, 11]]

    for n in (1, 2, 3, 17, 300):
        lr, sp_all, sp_kf, st = _answers(oracle, b"a" * n, 1)
        assert lr == ([n - 1] + list(range(n - 1, 0, -1)) if n > 1 else [0])
        assert sp_all == ([[0, n]] if n > 1 else []) and sp_kf == ([[1, n]] if n > 1 else [])
        assert st["longest"] == n - 1 and st["longest_pos"] == (0 if n > 1 else -1)
        assert st["lcp_sum"] == n * (n - 1) // 2 and st["distinct_substrings"] == n
        for k in (n - 1, n):
            if k >= 1:
                _, a, f, _ = _answers(oracle, b"a" * n, k)
                assert a == ([[0, n]] if k <= n - 1 else []) and f == ([[1, n]] if k <= n - 1 else [])
    assert _answers(oracle, b"", 1) == ([], [], [], {"longest": 0, "longest_pos": -1, "lcp_sum": 0, "distinct_substrings": 0,
                                                      "spans": 0, "covered_bytes": 0, "flagged": 0})


# ---------------------------------------------------------------- the interface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_REPEATS_ALL\s+0\b", header)
    assert re.search(r"#define\s+SA_AMD_REPEATS_KEEP_FIRST\s+1\b", header)
    assert "sa_amd_repeat_stats" in header
    for field in ("longest", "longest_pos", "lcp_sum", "distinct_substrings", "spans", "covered_bytes", "flagged", "readbacks"):
        assert field in dict(sa.RepeatStats._fields_), field
    assert ctypes.sizeof(sa.RepeatStats) == 64


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(sa.repeat_lengths) == ["s", "sa"]
    assert inspect.signature(sa.repeat_lengths).parameters["sa"].default is None
    assert params(sa.repeat_spans) == ["s", "min_len", "keep_first", "sa"]
    sig = inspect.signature(sa.repeat_spans).parameters
    assert sig["keep_first"].default is False and sig["sa"].default is None
    assert params(sa.last_repeat_stats) == [] and params(sa.repeats_work_bytes) == ["n"]
    assert params(sa.repeat_lengths_device_ptr)[:6] == ["text_ptr", "sa_ptr", "n", "lr_ptr", "work_ptr", "work_bytes"]
    assert params(sa.repeat_spans_device_ptr)[:9] == ["text_ptr", "sa_ptr", "n", "min_len", "mode", "spans_ptr", "capacity", "work_ptr",
                                                     "work_bytes"]
    assert params(sa.DeviceIndex.repeat_lengths) == ["self"] and params(sa.DeviceIndex.repeat_spans) == ["self", "min_len", "keep_first"]
    assert params(sa.SuffixArray.repeat_lengths) == ["self"] and params(sa.SuffixArray.repeat_spans) == ["self", "min_len", "keep_first"]
    assert (sa.REPEATS_ALL, sa.REPEATS_KEEP_FIRST) == (0, 1)
    for name in ("repeat_lengths", "repeat_spans", "last_repeat_stats", "repeats_work_bytes", "repeat_lengths_device_ptr",
                 "repeat_spans_device_ptr"):
        assert name in sa.__all__


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.zeros(256, dtype=np.uint32)
    p = buf.ctypes.data
    p256 = (p + 255) & ~255
    cnt = ctypes.c_int64(-7)
    c = ctypes.byref(cnt)
    big = 1 << 30
    assert L.sa_amd_repeats_work_bytes(-1) == -1
    assert L.sa_amd_repeat_spans_bound(-1, 5) == -1 and L.sa_amd_repeat_spans_bound(10, 0) == -1
    assert L.sa_amd_repeat_lengths(None, -1, None, p) == -1                                   # n < 0
    assert L.sa_amd_repeat_lengths(None, 4, None, p) == -1                                    # null text
    assert L.sa_amd_repeat_lengths(p, 4, p, None) == -1                                       # null output
    assert L.sa_amd_repeat_spans(p, 4, p, 0, 0, p, 4, c) == -1                                # min_len < 1
    assert L.sa_amd_repeat_spans(p, 4, p, -3, 1, p, 4, c) == -1
    assert L.sa_amd_repeat_spans(p, 4, p, 2, 2, p, 4, c) == -1                                # unknown mode
    assert L.sa_amd_repeat_spans(p, 4, p, 2, -1, p, 4, c) == -1
    assert L.sa_amd_repeat_spans(p, 4, p, 2, 0, p, -1, c) == -1                               # negative capacity
    assert L.sa_amd_repeat_spans(p, 4, p, 2, 0, None, 4, c) == -1                             # null output with room asked for
    assert L.sa_amd_repeat_spans(p, 4, p, 2, 0, p, 4, None) == -1                             # null count
    assert L.sa_amd_repeat_spans(None, 4, p, 2, 0, p, 4, c) == -1
    assert L.sa_amd_repeat_lengths_device(p, p, -1, p, p256, big, None) == -1
    assert L.sa_amd_repeat_lengths_device(p, None, 4, p, p256, big, None) == -1
    assert L.sa_amd_repeat_lengths_device(p, p, 4, None, p256, big, None) == -1
    assert L.sa_amd_repeat_lengths_device(p, p, 4, p, None, big, None) == -1
    assert L.sa_amd_repeat_lengths_device(None, p, 4, p, p256, big, None) == -1
    assert L.sa_amd_repeat_lengths_device(p, p, 4, p, p256 + 4, big, None) == -1              # misaligned work
    assert L.sa_amd_repeat_lengths_device(p, p, 4, p, p256, 16, None) == -1                   # short work
    assert L.sa_amd_repeat_spans_device(p, p, 4, 0, 0, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_repeat_spans_device(p, p, 4, 2, 7, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_repeat_spans_device(p, p, 4, 2, 0, p, -1, c, p256, big, None) == -1
    assert L.sa_amd_repeat_spans_device(p, p, 4, 2, 0, p, 4, None, p256, big, None) == -1
    assert L.sa_amd_repeat_spans_device(p, p, 4, 2, 0, None, 4, c, p256, big, None) == -1
    assert L.sa_amd_repeat_spans_device(p, p, 4, 2, 0, p, 4, c, p256 + 8, big, None) == -1
    assert L.sa_amd_index_repeat_lengths(None, p) == -1
    assert L.sa_amd_index_repeat_spans(None, 2, 0, p, 4, c) == -1
    assert cnt.value == -7 and not buf.any()                                                  # nothing written
    st = sa.RepeatStats()
    L.sa_amd_last_repeat_stats(ctypes.byref(st))
    L.sa_amd_last_repeat_stats(None)
    with pytest.raises(ValueError):
        sa.repeat_spans(b"abcabc", 0)
    with pytest.raises(ValueError):
        sa.repeat_spans_bound(6, 0)


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 4096, 1 << 20, (1 << 30) + 4097, 2**31 - 1])
def test_work_block_and_span_bound(n):
    """the work block is the LCP array's plus one n-entry buffer: within the streaming integrity check's block plus the two
    n-entry buffers"""
    L = sa.lib()
    w = L.sa_amd_repeats_work_bytes(n)
    assert w == L.sa_amd_lcp_work_bytes(n) + (4 * (n + 1) + 255) // 256 * 256
    assert w <= L.sa_amd_check_integrity_work_bytes(n) + 8 * (n + 1) + 256
    assert w % 256 == 0
    for k in (1, 2, 50, 2**31 - 1):
        assert L.sa_amd_repeat_spans_bound(n, k) == (n + 1) // (k + 1) == sa.repeat_spans_bound(n, k)
