"""CPU suite for the document frequency of the repeated substrings: the definitions of include/suffix_array_amd.h restated in numpy
(the nodes of test_substrings_abi, the pairs of neighbouring occurrences of one document, an argmin of LCP per pair, the scanned
table E, df = count - (E[hi] - E[lo + 1]), the query with the order by df and its tie rule), checked against literal counting
of the documents of every substring's occurrences and the known answers; a replica of the kernels' walk through the fan-out-32
minima with its load bound; the exports, the structure layouts, the ctypes signatures, the Python surface and the argument
checks that answer without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT
from test_substrings_abi import ALL, BY_COUNT, BY_COVER, BY_LENGTH, naive_arrays, node_table, run_query

EXPORTS = ("sa_amd_doc_substrings_work_bytes", "sa_amd_index_doc_substrings", "sa_amd_last_doc_substr_stats")
BY_DOCS = 4
FAN = 32


# ---------------------------------------------------------------- the model ----

def slot_docs(arr, doc_off):
    """doc(SA[i]) for every slot, -1 for slot 0 (the empty suffix): the last d with doc_off[d] <= SA[i]"""
    arr = np.asarray(arr, dtype=np.int64)
    off = np.asarray(doc_off, dtype=np.int64)
    d = np.searchsorted(off, arr, side="right") - 1
    d[arr >= off[-1]] = -1
    return d


def prev_slots(docs):
    """P[i] = the previous slot of the document of slot i, -1 where there is none (and for slot 0)"""
    docs = np.asarray(docs, dtype=np.int64)
    order = np.argsort(docs, kind="stable")
    P = np.full(docs.size, -1, dtype=np.int64)
    same = (docs[order][1:] == docs[order][:-1]) & (docs[order][1:] >= 0)
    P[order[1:][same]] = order[:-1][same]
    return P


def range_argmin(a, l, r, pick="left"):
    """an argmin of a over [l, r] (inclusive) for arrays of ranges, by a sparse table; pick: which of two equal halves wins"""
    a = np.asarray(a, dtype=np.int64)
    l = np.asarray(l, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    levels = [np.arange(a.size, dtype=np.int64)]
    span = 1
    while 2 * span <= a.size:
        x, y = levels[-1][:-span], levels[-1][span:]
        levels.append(np.where(a[y] < a[x], y, x) if pick == "left" else np.where(a[y] <= a[x], y, x))
        span *= 2
    out = np.zeros(l.size, dtype=np.int64)
    if not l.size:
        return out
    k = np.floor(np.log2(r - l + 1)).astype(np.int64)
    k -= (1 << k) > (r - l + 1)
    k += (2 << k) <= (r - l + 1)
    for j in np.unique(k).tolist():
        sel = k == j
        x, y = levels[j][l[sel]], levels[j][r[sel] - (1 << j) + 1]
        out[sel] = np.where(a[y] < a[x], y, x) if pick == "left" else np.where(a[y] <= a[x], y, x)
    return out


def pair_table(lcp, P, pick="left", rng=None):
    """E (n + 2 entries) and the pair counters.  pick: "left", "right", or "random" (a random argmin per pair: slow, small texts)"""
    lcp = np.asarray(lcp, dtype=np.int64)
    n = lcp.size - 1
    i = np.nonzero(P >= 0)[0]
    p = P[i]
    if pick == "random":
        m = np.array([rng.choice(np.nonzero(lcp[a + 1:b + 1] == lcp[a + 1:b + 1].min())[0]) + a + 1 for a, b in zip(p.tolist(), i.tolist())],
                     dtype=np.int64)
    else:
        m = range_argmin(lcp, p + 1, i, pick)
    assert ((m > p) & (m <= i)).all()
    G = np.bincount(m, minlength=n + 2)[:n + 2]
    E = np.concatenate(([0], np.cumsum(G)))[:n + 2]
    return E, {"pairs": int(i.size), "rmq_far": int((((p + 1) // FAN) != (i // FAN)).sum())}


def node_df(tab, E):
    lo, count = tab["lo"], tab["count"]
    return count - (E[lo + count] - E[lo + 1])


def doc_table(lcp, arr, doc_off, pick="left", rng=None):
    """node_table with the column df and the pair counters"""
    tab = dict(node_table(lcp))
    E, st = pair_table(lcp, prev_slots(slot_docs(arr, doc_off)), pick, rng)
    tab["df"] = node_df(tab, E)
    tab.update(st)
    return tab


def run_doc_query(tab, min_len=1, max_len=0, min_count=2, min_docs=1, order=ALL, k=0):
    """-> (rows (r, 4) uint32, df (r) uint32, representative slots, counters)"""
    depth, parent, count, df = tab["depth"], tab["parent"], tab["count"], tab["df"]
    sel = (depth >= min_len) & (count >= min_count) & (df >= min_docs)
    if max_len:
        sel &= parent < max_len
    length = np.minimum(depth, max_len) if max_len else depth
    stats = {"nodes": int(depth.size), "selected": int(sel.sum()),
             "distinct_selected": int((length - np.maximum(parent, min_len - 1))[sel].sum()),
             "df_sum": int(df[sel].sum()), "max_df": int(df[sel].max()) if sel.any() else 0,
             "pairs": tab["pairs"], "rmq_far": tab["rmq_far"]}
    idx = np.nonzero(sel)[0]
    if order != ALL:
        key = {BY_COUNT: count, BY_LENGTH: length, BY_COVER: count * length, BY_DOCS: df}[order][idx]
        idx = idx[np.lexsort((tab["slot"][idx], -key))][:k]           # key descending, equal keys by slot ascending
    rows = np.stack([tab["lo"][idx], count[idx], depth[idx], parent[idx]], axis=1).astype(np.uint32).reshape(-1, 4)
    return rows, df[idx].astype(np.uint32), tab["slot"][idx], stats


# the kernels' walk (kernels/doc_substrings.hpp, lz_rmq_query), word for word: the levels, the argmin it returns, the words it loads

def minima_levels(a):
    """[level 0 = a, level 1, ...]: level k = minima over 32^k entries; the top is the first level k >= 2 with at most 32 entries"""
    levels = [np.asarray(a, dtype=np.int64)]
    while True:
        cur = levels[-1]
        pad = (-cur.size) % FAN
        levels.append(np.concatenate((cur, np.full(pad, 1 << 40))).reshape(-1, FAN).min(axis=1))
        if len(levels) - 1 >= 2 and levels[-1].size <= FAN:
            return levels


def rmq_walk(levels, l, r):
    """-> (argmin slot, words loaded)"""
    level, blevel, a, b, bnode, best, steps = 0, 0, l, r + 1, l, 1 << 62, 0

    def scan(js):
        nonlocal best, bnode, blevel, steps
        for j in js:
            steps += 1
            if levels[level][j] < best:
                best, bnode, blevel = int(levels[level][j]), j, level
    while True:
        if a // FAN == (b - 1) // FAN:
            scan(range(a, b))
            break
        if a % FAN:
            scan(range(a, (a | (FAN - 1)) + 1))
            a = (a | (FAN - 1)) + 1
        if b % FAN:
            scan(range(b - b % FAN, b))
            b -= b % FAN
        a, b, level = a // FAN, b // FAN, level + 1
        if a >= b:
            break
    while blevel > 0:
        blevel -= 1
        first = bnode * FAN
        last = min(first + FAN - 1, levels[blevel].size - 1)
        c = first
        while c < last:
            steps += 1
            if levels[blevel][c] <= best:
                break
            c += 1
        bnode = c
    return bnode, steps


def rmq_bound(n):
    """93 K + 32 words a query, K the number of levels of minima over the n + 1 entries of LCP"""
    size, k = n + 1, 0
    while True:
        size, k = -(-size // FAN), k + 1
        if k >= 2 and size <= FAN:
            return 93 * k + 32


def walk_counters(lcp, P):
    """rmq_steps and rmq_max of the pair pass, and G as the walk's choices give it"""
    levels = minima_levels(lcp)
    n = len(lcp) - 1
    G = np.zeros(n + 2, dtype=np.int64)
    total = worst = 0
    for i in np.nonzero(P >= 0)[0].tolist():
        m, s = rmq_walk(levels, int(P[i]) + 1, i)
        G[m] += 1
        total, worst = total + s, max(worst, s)
    return {"rmq_steps": total, "rmq_max": worst}, np.concatenate(([0], np.cumsum(G)))[:n + 2]


# ---------------------------------------------------------------- model against literal counting ----

def literal_df(b, doc_off, arr, tab):
    """per node: the set of documents of the occurrences of its substring, found by comparing the text"""
    off = np.asarray(doc_off, dtype=np.int64)
    out = []
    for lo, depth in zip(tab["lo"].tolist(), tab["depth"].tolist()):
        sub = b[int(arr[lo]):int(arr[lo]) + depth]
        where = [q for q in range(len(b)) if b[q:q + depth] == sub]
        out.append(len({int(np.searchsorted(off, q, side="right") - 1) for q in where}))
    return np.asarray(out, dtype=np.int64)


def random_collection(rng, n):
    ndocs = int(rng.integers(1, 7))
    cuts = np.sort(rng.integers(0, n + 1, ndocs - 1)) if ndocs > 1 else np.zeros(0, dtype=np.int64)
    return np.concatenate(([0], cuts, [n])).astype(np.int64)              # equal cuts: empty documents, at either end too


def test_model_against_literal_counting_on_random_texts():
    rng = np.random.default_rng(20)
    texts = nodes = 0
    for sigma in (1, 2, 3):
        for _ in range(110):
            n = int(rng.integers(0, 41))
            b = bytes(rng.integers(97, 97 + sigma, n, dtype=np.uint8))
            off = random_collection(rng, n)
            arr, lcp = naive_arrays(b)
            want = None
            for pick in ("left", "right", "random"):
                tab = doc_table(lcp, arr, off, pick, rng)
                want = literal_df(b, off, arr, tab) if want is None else want
                assert np.array_equal(tab["df"], want), (b, off.tolist(), pick)
            nonempty = int((np.diff(off) > 0).sum())
            assert ((tab["df"] >= 1) & (tab["df"] <= np.minimum(tab["count"], max(nonempty, 1)))).all()
            assert tab["pairs"] == n - nonempty
            cnt, E = walk_counters(lcp, prev_slots(slot_docs(arr, off)))      # the kernels' own choice of argmin
            assert np.array_equal(node_df(tab, E), want) and cnt["rmq_max"] <= rmq_bound(n)
            texts += 1
            nodes += want.size
    assert texts >= 300 and nodes > 3000


def test_walk_returns_an_argmin_within_its_load_bound():
    rng = np.random.default_rng(21)
    for n, hi in ((1, 3), (31, 3), (32, 2), (33, 5), (1023, 2), (1025, 4), (33000, 3)):
        a = rng.integers(0, hi, n + 1)
        levels = minima_levels(a)
        assert len(levels) - 1 >= 2 and levels[-1].size <= FAN
        ls = rng.integers(0, n + 1, 300)
        rs = rng.integers(0, n + 1, 300)
        for l, r in zip(np.minimum(ls, rs).tolist(), np.maximum(ls, rs).tolist()):
            m, steps = rmq_walk(levels, l, r)
            assert l <= m <= r and a[m] == a[l:r + 1].min() and 1 <= steps <= rmq_bound(n), (n, l, r)
        m, steps = rmq_walk(levels, 0, n)                              # the whole array
        assert a[m] == a.min() and steps <= rmq_bound(n)
    assert rmq_bound(1 << 20) == 93 * 4 + 32 and rmq_bound(2**31 - 1) == 93 * 6 + 32 and rmq_bound(5) == 93 * 2 + 32
    assert np.array_equal(range_argmin([3, 1, 2, 1, 5], [0, 2, 4, 0], [4, 4, 4, 0], "left"), [1, 3, 4, 0])
    assert np.array_equal(range_argmin([3, 1, 2, 1, 5], [0, 2, 4, 0], [4, 4, 4, 0], "right"), [3, 3, 4, 0])


def _by_substring(b, off):
    arr, lcp = naive_arrays(b)
    tab = doc_table(lcp, arr, off)
    return {b[int(arr[lo]):int(arr[lo]) + d]: (int(c), int(f)) for lo, c, d, f in zip(tab["lo"], tab["count"], tab["depth"], tab["df"])}, tab


def test_known_answers():
    got, tab = _by_substring(b"abracadabra", [0, 4, 4, 7, 11])
    assert got == {b"a": (5, 3), b"abra": (2, 2), b"bra": (2, 2), b"ra": (2, 2)}
    rows, df, _, st = run_doc_query(tab, order=BY_DOCS, k=2)
    assert rows.tolist() == [[1, 5, 1, 0], [2, 2, 4, 1]] and df.tolist() == [3, 2]       # "a", then the first of the df = 2 nodes by slot
    assert st["df_sum"] == 9 and st["max_df"] == 3 and st["pairs"] == 11 - 3
    assert run_doc_query(tab, min_docs=3)[0].tolist() == [[1, 5, 1, 0]] and run_doc_query(tab, min_docs=4)[0].shape == (0, 4)
    assert run_doc_query(tab, min_docs=2, order=BY_LENGTH, k=1)[0].tolist() == [[2, 2, 4, 1]]      # longest common to two documents: "abra"
    got, tab = _by_substring(b"aaaa", [0, 2, 4])
    assert got == {b"a": (4, 2), b"aa": (3, 2), b"aaa": (2, 1)}
    assert run_doc_query(tab, min_docs=2, order=BY_LENGTH, k=1)[1].tolist() == [2]
    got, _ = _by_substring(b"aaaa", [0, 0, 4, 4])
    assert got == {b"a": (4, 1), b"aa": (3, 1), b"aaa": (2, 1)}


def test_equivalences():
    rng = np.random.default_rng(22)
    for _ in range(40):
        n = int(rng.integers(2, 60))
        b = bytes(rng.integers(97, 99, n, dtype=np.uint8))
        arr, lcp = naive_arrays(b)
        one = doc_table(lcp, arr, [0, n])
        assert (one["df"] == 1).all() and one["pairs"] == n - 1                       # one document
        every = doc_table(lcp, arr, np.arange(n + 1))
        assert np.array_equal(every["df"], every["count"]) and every["pairs"] == 0       # every byte its own document
        tab = doc_table(lcp, arr, random_collection(rng, n))
        plain = node_table(lcp)
        for flt in ((1, 0, 2), (2, 3, 2), (1, 1, 3)):
            for order, k in ((ALL, 0), (BY_COUNT, 3), (BY_LENGTH, 100), (BY_COVER, 1)):
                rows, _, slots, st = run_doc_query(tab, *flt, min_docs=1, order=order, k=k)
                exp, eslots, est = run_query(plain, *flt, order=order, k=k)
                assert np.array_equal(rows, exp) and np.array_equal(slots, eslots)
                assert all(st[key] == est[key] for key in ("nodes", "selected", "distinct_selected"))
        # text ++ text with the boundary in the middle: a node with an occurrence in either half has df = 2
        arr2, lcp2 = naive_arrays(b + b)
        tab2 = doc_table(lcp2, arr2, [0, n, 2 * n])
        for lo, c, f in zip(tab2["lo"].tolist(), tab2["count"].tolist(), tab2["df"].tolist()):
            where = arr2[lo:lo + c]
            assert f == int((where < n).any()) + int((where >= n).any())
        inner = np.array([(arr2[lo:lo + c] + d <= n).any() for lo, c, d in zip(tab2["lo"], tab2["count"], tab2["depth"])], dtype=bool)
        assert (tab2["df"][inner] == 2).all()                       # an occurrence inside the first half has its copy in the second


def test_order_by_docs_is_strict_with_ties_by_slot():
    b = b"abcabcxbcxabc"
    arr, lcp = naive_arrays(b)
    tab = doc_table(lcp, arr, [0, 3, 7, 10, 13])
    rows, df, slots, _ = run_doc_query(tab, order=BY_DOCS, k=100)
    key = df.astype(np.int64)
    assert (np.diff(key) <= 0).all() and np.unique(key).size < key.size
    for a in range(rows.shape[0] - 1):
        assert key[a] > key[a + 1] or slots[a] < slots[a + 1]
    assert np.array_equal(run_doc_query(tab, order=BY_DOCS, k=2)[0], rows[:2])


# ---------------------------------------------------------------- the interface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_SUBSTR_BY_DOCS\s+4\b", header) and sa.SUBSTR_BY_DOCS == 4
    for struct, cls, size in (("sa_amd_doc_substr_query", sa.DocSubstrQuery, 32), ("sa_amd_doc_substr_stats", sa.DocSubstrStats, 88),
                              ("sa_amd_substr_query", sa.SubstrQuery, 24)):                 # the old query keeps its layout
        body = header[header.index("typedef struct " + struct):]
        body = body[:body.index("} " + struct)]
        declared = re.findall(r"\bint(?:32|64)_t\s+(\w+)\s*;", body)
        assert declared == [name for name, _ in cls._fields_], struct
        for name, ctype in cls._fields_:
            assert re.search(r"\b" + ("int64_t" if ctype is ctypes.c_int64 else "int32_t") + r"\s+" + name + r"\s*;", body), name
        assert ctypes.sizeof(cls) == size
    assert [name for name, _ in sa.DocSubstrQuery._fields_] == ["min_len", "max_len", "min_count", "order", "k", "min_docs"]
    block = header[header.index("Repeated substrings with their document frequency"):]
    for text in ("df = count - (E[lo + count] - E[lo + 1])", "cross a document boundary", "sa_amd_last_substr_stats", "93 K + 32",
                 "no collection set", '"a" (count 5, df 3)'):
        assert text in block, text


def test_ctypes_signatures():
    L = sa.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.sa_amd_doc_substrings_work_bytes.argtypes == [i32] and L.sa_amd_doc_substrings_work_bytes.restype is i64
    assert L.sa_amd_index_doc_substrings.argtypes == [vp, vp, vp, vp, vp, i64, vp] and L.sa_amd_index_doc_substrings.restype is i32
    assert L.sa_amd_last_doc_substr_stats.argtypes == [vp] and L.sa_amd_last_doc_substr_stats.restype is None


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        sig = inspect.signature(cls.doc_substrings)
        assert params(cls.doc_substrings) == ["self", "min_len", "max_len", "min_count", "min_docs", "order", "k", "positions"]
        assert [sig.parameters[p].default for p in params(cls.doc_substrings)[1:]] == [1, 0, 2, 1, sa.SUBSTR_ALL, 0, False]
        assert "EXTENSION" in cls.doc_substrings.__doc__, cls.__name__
    assert params(sa.last_doc_substr_stats) == [] and params(sa.doc_substrings_work_bytes) == ["n"]
    for name in ("DocSubstrQuery", "DocSubstrStats", "SUBSTR_BY_DOCS", "last_doc_substr_stats", "doc_substrings_work_bytes"):
        assert name in sa.__all__, name
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        hpp = f.read()
    assert "struct DocSubstring" in hpp and "sa_amd_index_doc_substrings(" in hpp


def test_argument_checks_answer_without_a_device():
    """a NULL index is refused whatever else is passed, and nothing is written; the refusals that need an index (no collection,
    the query's ranges, the output arguments) are in the GPU suite"""
    L = sa.lib()
    buf = np.zeros(256, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-7)
    c = ctypes.byref(tot)
    for q in (sa.DocSubstrQuery(1, 0, 2, ALL, 0, 1), sa.DocSubstrQuery(1, 0, 2, BY_DOCS, 5, 2), sa.DocSubstrQuery(0, 0, 2, ALL, 0, 1),
              sa.DocSubstrQuery(1, 0, 2, 5, 1, 1), sa.DocSubstrQuery(1, 0, 2, ALL, 0, 0)):
        assert L.sa_amd_index_doc_substrings(None, ctypes.byref(q), p, p, p, 4, c) == -1
        assert L.sa_amd_index_doc_substrings(None, ctypes.byref(q), None, None, None, 0, c) == -1
    assert L.sa_amd_index_doc_substrings(None, None, p, p, p, 4, c) == -1
    assert L.sa_amd_index_doc_substrings(None, None, p, p, p, -1, None) == -1
    assert tot.value == -7 and not buf.any()                                                  # nothing written
    st = sa.DocSubstrStats()
    L.sa_amd_last_doc_substr_stats(ctypes.byref(st))
    L.sa_amd_last_doc_substr_stats(None)
    assert set(sa.last_doc_substr_stats()) == {name for name, _ in sa.DocSubstrStats._fields_}
    before = sa.last_substr_stats()
    assert sa.last_substr_stats() == before


SIZES = [0, 1, 2, 3, 31, 1000, 4096, 1 << 20, (1 << 20) + 4097, (1 << 30) + 4097, 2**31 - 1]


def test_work_block():
    """the substrings block plus one buffer of n + 2 entries; monotone"""
    L = sa.lib()
    assert L.sa_amd_doc_substrings_work_bytes(-1) == -1
    prev = 0
    for n in SIZES:
        w = L.sa_amd_doc_substrings_work_bytes(n)
        base = L.sa_amd_substrings_work_bytes(n)
        assert w % 256 == 0 and w == sa.doc_substrings_work_bytes(n)
        assert base + 4 * (n + 2) <= w <= base + 4 * (n + 68) + 256
        assert w >= prev
        prev = w
