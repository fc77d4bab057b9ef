"""CPU suite for repeated-substring enumeration: the definitions of include/suffix_array_amd.h restated in numpy (a stack pass over
the LCP array for the "<=" neighbour on the left and the "<" neighbour on the right, then rows, filter, the three keys with
their tie rule and the four counters), checked against literal substring counting and the known answers; the exports, the
ctypes signatures, the Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re
from collections import Counter

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, fibonacci_word
from test_lcp_abi import _kasai

EXPORTS = ("sa_amd_substrings_work_bytes", "sa_amd_substrings_bound", "sa_amd_substrings_device", "sa_amd_substrings",
           "sa_amd_index_substrings", "sa_amd_last_substr_stats")
ALL, BY_COUNT, BY_LENGTH, BY_COVER = 0, 1, 2, 3
TILE = 1024                                                          # slots per tile of the neighbour stage


# ---------------------------------------------------------------- the model ----

def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def neighbours(lcp):
    """stack pass over LCP[0 .. n]: (le, lt), the nearest j < i with LCP[j] <= LCP[i] and the nearest j > i with LCP[j] < LCP[i],
    -1 where there is none"""
    a = np.asarray(lcp, dtype=np.int64).tolist()
    m = len(a)
    le, lt = [-1] * m, [-1] * m
    st = []
    for i in range(m):
        while st and a[st[-1]] > a[i]:
            lt[st.pop()] = i
        if st:
            le[i] = st[-1]                                            # (what is left on the stack is <= a[i], the top the nearest)
        st.append(i)
    return np.asarray(le, dtype=np.int64), np.asarray(lt, dtype=np.int64)


def node_table(lcp):
    """every node of the LCP array (n + 1 entries) as int64 columns slot, lo, count, depth, parent, in slot order; `unresolved`:
    the slots with a neighbour that is not inside their tile"""
    lcp = np.asarray(lcp, dtype=np.int64)
    n = lcp.size - 1
    le, lt = neighbours(lcp)
    i = np.arange(n + 1, dtype=np.int64)
    rep = (i >= 2) & (lcp > 0) & (le >= 0) & (lcp[np.maximum(le, 0)] < lcp)
    slot = i[rep]
    lo = le[rep]
    hi = np.where(lt[rep] >= 0, lt[rep], n + 1)
    ext = np.append(lcp, 0)                                          # LCP[n + 1] read as 0
    outside = (le < 0) | (le // TILE != i // TILE) | (lt < 0) | (lt // TILE != i // TILE)
    return {"n": n, "slot": slot, "lo": lo, "count": hi - lo, "depth": lcp[slot], "parent": np.maximum(ext[lo], ext[hi]),
            "unresolved": int(outside.sum())}


def run_query(tab, min_len=1, max_len=0, min_count=2, order=ALL, k=0):
    """-> (rows (r, 4) uint32, representative slots, counters)"""
    depth, parent, count = tab["depth"], tab["parent"], tab["count"]
    sel = (depth >= min_len) & (count >= min_count)
    if max_len:
        sel &= parent < max_len
    length = np.minimum(depth, max_len) if max_len else depth
    stats = {"nodes": int(depth.size), "selected": int(sel.sum()), "distinct_all": int((depth - parent).sum()),
             "distinct_selected": int((length - np.maximum(parent, min_len - 1))[sel].sum())}
    idx = np.nonzero(sel)[0]
    if order != ALL:
        key = {BY_COUNT: count, BY_LENGTH: length, BY_COVER: count * length}[order][idx]
        idx = idx[np.lexsort((tab["slot"][idx], -key))][:k]           # key descending, equal keys by slot ascending
    rows = np.stack([tab["lo"][idx], count[idx], depth[idx], parent[idx]], axis=1).astype(np.uint32).reshape(-1, 4)
    return rows, tab["slot"][idx], stats


def naive_arrays(t):
    """suffix array (n + 1 entries, SA[0] = n) and LCP array of a short text, literally"""
    b = bytes(t)
    n = len(b)
    arr = sorted(range(n + 1), key=lambda p: b[p:])
    lcp = [0] * (n + 1)
    for i in range(1, n + 1):
        x, y = b[arr[i - 1]:], b[arr[i]:]
        h = 0
        while h < min(len(x), len(y)) and x[h] == y[h]:
            h += 1
        lcp[i] = h
    return np.asarray(arr, dtype=np.int64), np.asarray(lcp, dtype=np.int64)


def _check_against_counting(b, queries=()):
    """the statements of the header, literally: every substring that occurs twice lies in exactly one node with that count, a
    node's substring occurs at exactly SA[lo .. lo + count), and the counters count distinct substrings"""
    b = bytes(b)
    n = len(b)
    arr, lcp = naive_arrays(b)
    tab = node_table(lcp)
    occ = Counter(b[p:p + ln] for p in range(n) for ln in range(1, n - p + 1))
    repeated = {s: c for s, c in occ.items() if c >= 2}
    assert tab["slot"].size <= max(n - 1, 0)
    covered = {}
    for lo, count, depth, parent in zip(tab["lo"].tolist(), tab["count"].tolist(), tab["depth"].tolist(), tab["parent"].tolist()):
        assert lo >= 1 and count >= 2 and parent < depth
        p = int(arr[lo])
        sub = b[p:p + depth]
        where = sorted(q for q in range(n) if b[q:q + depth] == sub)
        assert where == sorted(arr[lo:lo + count].tolist())
        for ln in range(parent + 1, depth + 1):
            assert sub[:ln] not in covered                             # exactly one node
            covered[sub[:ln]] = count
    assert covered == repeated
    rows, _, st = run_query(tab)
    assert st["nodes"] == rows.shape[0] and st["distinct_all"] == len(repeated)
    for (mn, mx, mc) in queries:
        _, _, st = run_query(tab, mn, mx, mc)
        want = sum(1 for s, c in repeated.items() if c >= mc and len(s) >= mn and (mx == 0 or len(s) <= mx))
        assert st["distinct_selected"] == want, (b, mn, mx, mc)


def test_model_against_literal_counting_on_random_texts():
    rng = np.random.default_rng(19)
    texts = 0
    for sigma in (2, 3):
        for _ in range(160):
            n = int(rng.integers(0, 41))
            b = bytes(rng.integers(97, 97 + sigma, n, dtype=np.uint8))
            _check_against_counting(b, [(1, 0, 2), (2, 3, 2), (4, 4, 2), (1, 1, 3), (3, 0, 4)])
            texts += 1
    assert texts >= 300
    for b in (b"mississippi", b"banana", b"", b"a", b"aa", b"ab", b"abab", b"aaaaaaa"):
        _check_against_counting(b, [(1, 0, 2), (2, 3, 2)])


def test_banana_and_mississippi_rows():
    arr, lcp = naive_arrays(b"banana")
    assert lcp.tolist() == [0, 0, 1, 3, 0, 0, 2]
    tab = node_table(lcp)
    rows, slots, st = run_query(tab)
    assert rows.tolist() == [[1, 3, 1, 0], [2, 2, 3, 1], [5, 2, 2, 0]] and slots.tolist() == [2, 3, 6]
    assert arr[rows[:, 0]].tolist() == [5, 3, 4]
    assert st == {"nodes": 3, "selected": 3, "distinct_all": 5, "distinct_selected": 5}       # a, an, ana, n, na
    assert run_query(tab, order=BY_COUNT, k=1)[0].tolist() == [[1, 3, 1, 0]]
    assert run_query(tab, order=BY_LENGTH, k=2)[0].tolist() == [[2, 2, 3, 1], [5, 2, 2, 0]]
    assert run_query(tab, order=BY_COVER, k=5)[0].tolist() == [[2, 2, 3, 1], [5, 2, 2, 0], [1, 3, 1, 0]]       # 6, 4, 3
    assert run_query(tab, 1, 1, 2, BY_COVER, 5)[0].tolist() == [[1, 3, 1, 0], [5, 2, 2, 0]]                   # cut at 1: 3, 2
    assert run_query(tab, 1, 1, 3)[2]["distinct_selected"] == 1
    _, lcp = naive_arrays(b"mississippi")
    rows, _, st = run_query(node_table(lcp))
    # i x4, issi x2, p x2, s x4, si x2, ssi x2
    assert sorted(map(tuple, rows[:, 1:].tolist())) == sorted([(4, 1, 0), (2, 4, 1), (2, 1, 0), (4, 1, 0), (2, 2, 1), (2, 3, 1)])
    assert st["distinct_all"] == 1 + 3 + 1 + 1 + 1 + 2


def test_tie_rule_is_by_slot():
    tab = node_table(naive_arrays(b"abcabcxbcx")[1])
    rows, slots, _ = run_query(tab, order=BY_COUNT, k=100)
    key = rows[:, 1].astype(np.int64)
    assert (np.diff(key) <= 0).all()
    for a in range(rows.shape[0] - 1):
        assert key[a] > key[a + 1] or slots[a] < slots[a + 1]
    assert np.array_equal(run_query(tab, order=BY_COUNT, k=2)[0], rows[:2])


def _golden(name):
    gold = os.path.join(ROOT, "tests", "golden")
    return (np.fromfile(os.path.join(gold, name + ".text"), dtype=np.uint8),
            np.fromfile(os.path.join(gold, name + ".sa.u32le"), dtype="<u4"))


def test_model_on_the_golden_texts(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        names = sorted(json.load(f))
    assert names
    for name in names:
        t, arr = _golden(name)
        lcp = _kasai(oracle, t, arr).astype(np.int64)
        tab = node_table(lcp)
        n = t.size
        assert tab["slot"].size <= max(n - 1, 0)
        assert (tab["count"] >= 2).all() and (tab["parent"] < tab["depth"]).all() and (tab["lo"] >= 1).all()
        # the node of a representative is its LCP interval: everything inside is >= depth, both borders are smaller
        rng = np.random.default_rng(5)
        for r in rng.permutation(tab["slot"].size)[:200].tolist():
            lo, c, d = int(tab["lo"][r]), int(tab["count"][r]), int(tab["depth"][r])
            assert lcp[lo + 1:lo + c].min() == d and lcp[lo] < d and (lo + c > n or lcp[lo + c] < d)
            p, q = int(arr[lo]), int(arr[lo + c - 1])
            assert bytes(t[p:p + d]) == bytes(t[q:q + d])
        # sum over the nodes of (count - 1) * (depth - parent) = sum of LCP: every slot i > lo of a node shares depth - parent more
        assert int(((tab["count"] - 1) * (tab["depth"] - tab["parent"])).sum()) == int(lcp.sum())


def test_known_answers(oracle):
    def table(b):
        t = _u8(b)
        return node_table(_kasai(oracle, t, oracle.sais(t)))
    tab = table(b"a" * 1025)
    assert tab["slot"].size == 1024 and int(tab["depth"].max()) == 1024
    tab = table(b"ab" * 600)
    assert tab["slot"].size == 1198 and int(tab["depth"].max()) == 1198
    fib = fibonacci_word(15)
    assert len(fib) == 2584
    tab = table(fib)
    assert tab["slot"].size == 2579 and int(tab["depth"].max()) == 1595
    assert table(bytes(range(256)))["slot"].size == 0
    t, arr = _golden("all_bytes_twice")
    assert node_table(_kasai(oracle, t, arr))["slot"].size == 256


# ---------------------------------------------------------------- the interface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    for name, val in (("ALL", 0), ("BY_COUNT", 1), ("BY_LENGTH", 2), ("BY_COVER", 3)):
        assert re.search(r"#define\s+SA_AMD_SUBSTR_" + name + r"\s+" + str(val) + r"\b", header), name
        assert getattr(sa, "SUBSTR_" + name) == val
    for struct, cls, size in (("sa_amd_substr_query", sa.SubstrQuery, 24), ("sa_amd_substr_stats", sa.SubstrStats, 72)):
        body = header[header.index("typedef struct " + struct):]
        body = body[:body.index("} " + struct)]
        declared = re.findall(r"\bint(?:32|64)_t\s+(\w+)\s*;", body)
        assert declared == [name for name, _ in cls._fields_], struct
        for name, ctype in cls._fields_:
            assert re.search(r"\b" + ("int64_t" if ctype is ctypes.c_int64 else "int32_t") + r"\s+" + name + r"\s*;", body), name
        assert ctypes.sizeof(cls) == size
    for text in ("LCP[0] = LCP[1] = 0", "REPRESENTATIVE", "parent = max(LCP[lo], LCP[hi])", "sa_amd_last_lz_stats"):
        assert text in header[header.index("Repeated substrings (an extension)"):], text


def test_ctypes_signatures():
    L = sa.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.sa_amd_substrings_work_bytes.argtypes == [i32] and L.sa_amd_substrings_work_bytes.restype is i64
    assert L.sa_amd_substrings_bound.argtypes == [i32] and L.sa_amd_substrings_bound.restype is i64
    assert L.sa_amd_substrings_device.argtypes == [vp, vp, i32, vp, vp, vp, i64, vp, vp, i64, vp]
    assert L.sa_amd_substrings.argtypes == [vp, i32, vp, vp, vp, vp, i64, vp]
    assert L.sa_amd_index_substrings.argtypes == [vp, vp, vp, vp, i64, vp]
    for fn in (L.sa_amd_substrings_device, L.sa_amd_substrings, L.sa_amd_index_substrings):
        assert fn.restype is i32
    assert L.sa_amd_last_substr_stats.argtypes == [vp] and L.sa_amd_last_substr_stats.restype is None


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    sig = inspect.signature(sa.repeated_substrings)
    assert params(sa.repeated_substrings) == ["s", "min_len", "max_len", "min_count", "order", "k", "sa", "positions"]
    assert [sig.parameters[p].default for p in params(sa.repeated_substrings)[1:]] == [1, 0, 2, sa.SUBSTR_ALL, 0, None, False]
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.repeated_substrings) == ["self", "min_len", "max_len", "min_count", "order", "k", "positions"]
        assert "EXTENSION" in cls.repeated_substrings.__doc__, cls.__name__
    assert params(sa.last_substr_stats) == [] and params(sa.substrings_work_bytes) == ["n"] and params(sa.substrings_bound) == ["n"]
    assert params(sa.substrings_device_ptr)[:9] == ["text_ptr", "sa_ptr", "n", "query", "rows_ptr", "pos_ptr", "capacity", "work_ptr",
                                                    "work_bytes"]
    for name in ("repeated_substrings", "last_substr_stats", "substrings_work_bytes", "substrings_bound", "substrings_device_ptr",
                 "SubstrQuery", "SubstrStats", "SUBSTR_ALL", "SUBSTR_BY_COUNT", "SUBSTR_BY_LENGTH", "SUBSTR_BY_COVER"):
        assert name in sa.__all__, name
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        hpp = f.read()
    assert "struct RepeatedSubstring" in hpp and hpp.count("repeated_substrings(") >= 3


def _q(min_len=1, max_len=0, min_count=2, order=ALL, k=0):
    return sa.SubstrQuery(min_len, max_len, min_count, order, k)


BAD_QUERIES = [_q(min_len=0), _q(min_len=-3), _q(min_len=5, max_len=1), _q(min_len=5, max_len=4), _q(max_len=-1), _q(min_count=1),
               _q(min_count=0), _q(order=4), _q(order=-1), _q(order=BY_COUNT, k=0), _q(order=BY_LENGTH, k=-1), _q(order=BY_COVER, k=0)]


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.zeros(256, dtype=np.uint32)
    p = buf.ctypes.data
    p256 = (p + 255) & ~255
    tot = ctypes.c_int64(-7)
    c = ctypes.byref(tot)
    big = 1 << 30
    ok = _q()
    okp = ctypes.byref(ok)
    assert L.sa_amd_substrings_work_bytes(-1) == -1 and L.sa_amd_substrings_bound(-1) == -1
    for bad in BAD_QUERIES:
        b = ctypes.byref(bad)
        assert L.sa_amd_substrings(p, 4, p, b, p, p, 4, c) == -1, tuple(getattr(bad, f) for f, _ in bad._fields_)
        assert L.sa_amd_substrings(p, 4, None, b, p, None, 4, c) == -1
        assert L.sa_amd_substrings_device(p, p, 4, b, p, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_substrings(p, 4, p, None, p, p, 4, c) == -1                               # null query
    assert L.sa_amd_substrings(None, -1, p, okp, p, p, 4, c) == -1                            # n < 0
    assert L.sa_amd_substrings(None, 4, p, okp, p, p, 4, c) == -1                             # null text
    assert L.sa_amd_substrings(p, 4, p, okp, p, p, -1, c) == -1                               # negative capacity
    assert L.sa_amd_substrings(p, 4, p, okp, p, p, 4, None) == -1                             # null total
    assert L.sa_amd_substrings(p, 4, p, okp, None, p, 4, c) == -1                             # null rows with room asked for
    assert L.sa_amd_substrings_device(p, p, -1, okp, p, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_substrings_device(p, None, 4, okp, p, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_substrings_device(None, p, 4, okp, p, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_substrings_device(p, p, 4, okp, p, p, 4, c, None, big, None) == -1
    assert L.sa_amd_substrings_device(p, p, 4, okp, p, p, 4, c, p256 + 4, big, None) == -1    # misaligned work
    assert L.sa_amd_substrings_device(p, p, 4, okp, p, p, 4, c, p256, 64, None) == -1         # short work
    assert L.sa_amd_substrings_device(p, p, 4, okp, p, p, -1, c, p256, big, None) == -1
    assert L.sa_amd_substrings_device(p, p, 4, okp, p, p, 4, None, p256, big, None) == -1
    assert L.sa_amd_substrings_device(p, p, 4, okp, None, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_substrings_device(p, p, 4, None, p, p, 4, c, p256, big, None) == -1
    assert L.sa_amd_index_substrings(None, okp, p, p, 4, c) == -1
    assert tot.value == -7 and not buf.any()                                                  # nothing written
    with pytest.raises(ValueError):
        sa.repeated_substrings(b"banana", min_len=0)
    with pytest.raises(ValueError):
        sa.repeated_substrings(b"banana", order=sa.SUBSTR_BY_COUNT)                           # k = 0
    st = sa.SubstrStats()
    L.sa_amd_last_substr_stats(ctypes.byref(st))
    L.sa_amd_last_substr_stats(None)
    assert set(sa.last_substr_stats()) == {name for name, _ in sa.SubstrStats._fields_}


SIZES = [0, 1, 2, 3, 31, 1000, 4096, 1 << 20, (1 << 20) + 4097, (1 << 30) + 4097, 2**31 - 1]


def test_work_block_and_bound():
    """the LCP array's block plus five n-entry buffers; both functions are monotone"""
    L = sa.lib()
    prev_w, prev_b = 0, 0
    for n in SIZES:
        w, b = L.sa_amd_substrings_work_bytes(n), L.sa_amd_substrings_bound(n)
        assert w % 256 == 0 and w == sa.substrings_work_bytes(n) and b == sa.substrings_bound(n) == max(n - 1, 0)
        assert w >= L.sa_amd_lcp_work_bytes(n)
        assert L.sa_amd_lcp_work_bytes(n) + 20 * n <= w <= L.sa_amd_lcp_work_bytes(n) + 20 * (n + 68) + 4 * 256
        assert w >= prev_w and b >= prev_b
        prev_w, prev_b = w, b
