"""CPU suite for document collections over the index: the definitions of include/suffix_array_amd.h (doc, occ, df, the listing in
first-slot order, the stored per-slot word) restated in numpy over the oracle's suffix array and checked against literal brute
force; the exports, the Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases

EXPORTS = ("sa_amd_docs_work_bytes", "sa_amd_index_set_documents", "sa_amd_index_doc_of", "sa_amd_index_doc_of_device",
           "sa_amd_index_doc_search", "sa_amd_index_doc_list", "sa_amd_last_docs_stats", "sa_amd_docs_set_chunk")
NONE = 0xFFFFFFFF
EXAMPLE_TEXT = b"abracadabra"
EXAMPLE_OFF = [0, 4, 4, 7, 11]                                        # "abra", "", "cad", "abra"


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


# ---------------------------------------------------------------- the definitions ----

def doc_of_definition(doc_off, n, pos):
    """doc(p): the d with doc_off[d] <= p < doc_off[d + 1]; NONE for p >= n"""
    pos = np.asarray(pos, dtype=np.int64)
    d = np.searchsorted(np.asarray(doc_off, dtype=np.int64), pos, "right") - 1
    return np.where(pos >= n, NONE, d).astype(np.int64)


def range_definition(tb, arr, pat):
    """[lo, hi): the slots whose suffix starts with pat (search_all in the SA[0 .. n] layout); an absent pattern gives lo == hi"""
    k = len(pat)
    lo, hi = 0, len(arr)
    while lo < hi:                                                    # first slot whose suffix is not smaller than pat
        mid = (lo + hi) // 2
        p = int(arr[mid])
        if tb[p:p + k] < pat:
            lo = mid + 1
        else:
            hi = mid
    first = lo
    hi = len(arr)
    while lo < hi:                                                    # first slot behind it whose suffix does not start with pat
        mid = (lo + hi) // 2
        p = int(arr[mid])
        if tb[p:p + k] == pat:
            lo = mid + 1
        else:
            hi = mid
    return first, lo


def listing_definition(doc_off, n, arr, lo, hi):
    """the distinct documents of the slots [lo, hi), each once, in the order of the slot of their first occurrence"""
    d = doc_of_definition(doc_off, n, np.asarray(arr[lo:hi], dtype=np.int64))
    d = d[d != NONE]
    uniq, first = np.unique(d, return_index=True)
    return uniq[np.argsort(first, kind="stable")].astype(np.int64)


def word_definition(doc_off, n, arr):
    """the stored word per slot: previous slot of the same document + 1, 0 where there is none, 0xffffffff in slot 0"""
    da = doc_of_definition(doc_off, n, np.asarray(arr[1:], dtype=np.int64))
    order = np.argsort(da, kind="stable")                             # the slots less one, by document, slots ascending inside
    w = np.zeros(n + 1, dtype=np.int64)
    w[0] = NONE
    same = da[order[1:]] == da[order[:-1]]
    w[order[1:][same] + 1] = order[:-1][same] + 2
    return w


def answers_definition(tb, doc_off, arr, pats):
    """-> (occ, df, listings) of every pattern; df both from the listing and from the stored word's one compare"""
    n = len(tb)
    w = word_definition(doc_off, n, arr)
    occ, df, lists = [], [], []
    for pat in pats:
        lo, hi = range_definition(tb, arr, pat)
        ls = listing_definition(doc_off, n, arr, lo, hi)
        assert int(np.count_nonzero(w[lo:hi] <= lo)) == ls.size
        occ.append(hi - lo)
        df.append(ls.size)
        lists.append(ls)
    return np.array(occ, dtype=np.int64), np.array(df, dtype=np.int64), lists


def units_definition(occ, chunk):
    return int(sum((int(c) + chunk - 1) // chunk for c in occ))


# ---------------------------------------------------------------- brute force ----

def brute_suffix_rank(tb):
    """rank of every suffix, the empty one included, by sorting the suffixes themselves as bytes (no suffix array involved)"""
    order = sorted(range(len(tb) + 1), key=lambda s: tb[s:])
    rank = [0] * (len(tb) + 1)
    for r, s in enumerate(order):
        rank[s] = r
    return rank


def brute_starts(tb, pat, rank):
    """bytes.find from every start; the starts in the order of their suffixes"""
    n = len(tb)
    starts, p = [], tb.find(pat)
    while p >= 0:
        starts.append(p)
        p = tb.find(pat, p + 1)
    if not pat and (not starts or starts[-1] != n):
        starts.append(n)                                              # (the empty suffix; bytes.find reports it already for b"")
    starts.sort(key=rank.__getitem__)
    return np.array(starts, dtype=np.int64)


def brute_answers(doc_off, n, starts):
    """-> (occ, the listing): np.searchsorted(doc_off, p, 'right') - 1 of every start inside the text, each document once, in
    the order the sorted starts meet it"""
    inside = starts[starts < n]
    d = np.searchsorted(np.asarray(doc_off, dtype=np.int64), inside, "right") - 1
    return int(starts.size), list(dict.fromkeys(d.tolist()))


def brute_word(doc_off, n, arr):
    w = [NONE]
    for i in range(1, n + 1):
        d = int(np.searchsorted(np.asarray(doc_off, dtype=np.int64), int(arr[i]), "right") - 1)
        prev = 0
        for j in range(i - 1, 0, -1):
            if int(np.searchsorted(np.asarray(doc_off, dtype=np.int64), int(arr[j]), "right") - 1) == d:
                prev = j + 1
                break
        w.append(prev)
    return np.array(w, dtype=np.int64)


def offset_tables(n, rng):
    """offset tables of every shape the header allows for a text of n bytes"""
    out = {"one": [0, n], "every_byte": list(range(n + 1))}
    for k in (2, 3, 7):
        cuts = np.sort(rng.integers(0, n + 1, k - 1)).tolist()
        out["random%d" % k] = [0] + cuts + [n]
    out["empty_first"] = [0, 0, 0] + [n // 2, n]
    out["empty_last"] = [0, n // 3, n, n, n]
    out["empty_runs"] = [0, n // 4, n // 4, n // 4, n // 2, n // 2, n]
    out["more_docs_than_bytes"] = sorted(rng.integers(0, n + 1, 2 * n + 3).tolist() + [0, n])
    return out


def patterns_of(tb, rng, count=12):
    n = len(tb)
    pats = [b"", b"\x01\x02\x03nope"]
    for _ in range(count):
        if n:
            a = int(rng.integers(0, n))
            pats.append(tb[a:a + int(rng.integers(1, 6))])
    pats += [bytes([c]) for c in sorted(set(tb))[:4]]
    if n:
        pats.append(tb)
    return pats


def _brute_check(tb, oracle, rng, tables=None):
    """every table shape (or `tables`) over one text, the same patterns under each"""
    n = len(tb)
    arr = oracle.sais(_u8(tb))
    rank = brute_suffix_rank(tb)
    assert [rank[int(p)] for p in arr] == list(range(n + 1))
    pats = patterns_of(tb, rng)
    starts = [brute_starts(tb, pat, rank) for pat in pats]
    for name, off in (tables or offset_tables(n, rng)).items():
        offa = np.asarray(off, dtype=np.int64)
        assert off[0] == 0 and off[-1] == n and np.all(np.diff(offa) >= 0), name
        pos = np.concatenate([np.arange(n + 3), [NONE]])
        d = doc_of_definition(off, n, pos)
        assert np.all(d[n:] == NONE)
        assert np.all(offa[d[:n]] <= pos[:n]) and np.all(pos[:n] < offa[d[:n] + 1]), name
        if n <= 80:
            assert np.array_equal(word_definition(off, n, arr), brute_word(off, n, arr)), name
        occ, df, lists = answers_definition(tb, off, arr, pats)
        for q, pat in enumerate(pats):
            bo, bl = brute_answers(off, n, starts[q])
            assert (occ[q], lists[q].tolist()) == (bo, bl), (name, pat[:16])
            assert df[q] == len(bl) <= min(bo, len(off) - 1)
        assert occ[0] == n + 1 and df[0] == np.count_nonzero(np.diff(offa))


def test_the_header_example(oracle):
    tb, off = EXAMPLE_TEXT, EXAMPLE_OFF
    arr = oracle.sais(_u8(tb))
    occ, df, lists = answers_definition(tb, off, arr, [b"a", b"bra", b"", b"cad", b"zz"])
    assert occ.tolist() == [5, 2, 12, 1, 0] and df.tolist() == [3, 2, 3, 1, 0]
    assert lists[0].tolist() == [3, 0, 2] and lists[1].tolist() == [3, 0] and lists[3].tolist() == [2] and lists[4].tolist() == []
    assert arr[1:6].tolist() == [10, 7, 0, 3, 5]
    assert doc_of_definition(off, 11, [0, 3, 4, 6, 7, 10, 11, NONE]).tolist() == [0, 0, 2, 2, 3, 3, NONE, NONE]
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    assert '"a" has occ 5, df 3 and the listing\n *       {3, 0, 2}' in header
    _brute_check(tb, oracle, np.random.default_rng(1), {"example": off})


def test_definitions_against_brute_force_random(oracle):
    rng = np.random.default_rng(16)
    for trial in range(60):
        n = int(rng.integers(0, 50))
        sigma = int(rng.choice([1, 2, 3, 4, 26]))
        _brute_check(rng.integers(97, 97 + sigma, n).astype(np.uint8).tobytes(), oracle, rng)


def test_definitions_against_brute_force_golden(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        manifest = json.load(f)
    names = sorted(manifest)
    rng = np.random.default_rng(17)
    for name in names:
        with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
            tb = f.read()
        assert len(tb) == manifest[name]["n"]
        _brute_check(tb, oracle, rng)                                 # every table shape on every golden text
    assert len(names) >= 5


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_definitions_against_brute_force_adversarial(oracle, name):
    """every adversarial case of conftest under every table shape: random tables, one document, one per byte, empty documents
    first, last and in runs, more documents than bytes"""
    tb = adversarial_cases()[name]
    _brute_check(tb, oracle, np.random.default_rng(len(tb)))


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_DOC_NONE\s+0xffffffffu\b", header)
    assert sa.DOC_NONE == NONE == sa.MATCH_NONE
    body = header[header.index("typedef struct sa_amd_docs_stats"):]
    for field in ("patterns", "occ_sum", "units", "df_sum", "slots_scanned", "chunk", "readbacks", "listed"):
        assert field in dict(sa.DocsStats._fields_), field
        assert re.search(r"\b" + field + r"\b", body), field
    assert ctypes.sizeof(sa.DocsStats) == 5 * 8 + 4 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "docs.hpp")) as f:
        kernels = f.read()
    for name in ("DOC_SAMPLES", "DOC_CHUNK_MIN", "DOC_CHUNK_MAX", "DOC_CHUNK_DEFAULT"):
        m = re.search(r"constexpr int " + name + r" = ([^;]+);", kernels)
        assert m and eval(m.group(1)) == getattr(sa, name), name      # noqa: S307 (an integer expression of the project's own source)


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.set_documents) == ["self", "offsets"]
        assert params(cls.doc_of) == ["self", "positions"]
        assert params(cls.doc_search) == ["self", "patterns"]
        assert params(cls.doc_list) == ["self", "patterns"]
    assert params(sa.doc_of_device_ptr) == ["index", "pos_ptr", "count", "doc_ptr", "stream"]
    assert params(sa.docs_set_chunk) == ["slots"] and params(sa.docs_work_bytes) == ["n"]
    for name in ("DocsStats", "last_docs_stats", "docs_set_chunk", "docs_work_bytes", "doc_of_device_ptr", "DOC_NONE", "DOC_SAMPLES",
                 "DOC_CHUNK_MIN", "DOC_CHUNK_MAX", "DOC_CHUNK_DEFAULT"):
        assert name in sa.__all__ and hasattr(sa, name), name


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    offs = np.array([0, 2, 4], dtype=np.uint32)
    assert L.sa_amd_docs_work_bytes(-1) == -1
    assert L.sa_amd_index_set_documents(None, offs.ctypes.data, 2) == -1                        # NULL index
    assert L.sa_amd_index_doc_of(None, p, 4, p) == -1
    assert L.sa_amd_index_doc_of_device(None, p, 4, p, None) == -1
    assert L.sa_amd_index_doc_search(None, p, good.ctypes.data, 2, p, p) == -1
    assert L.sa_amd_index_doc_list(None, p, good.ctypes.data, 2, p, p, 4, c) == -1
    assert L.sa_amd_index_set_documents(fake, None, 2) == -1                                    # malformed doc_off
    assert L.sa_amd_index_set_documents(fake, offs.ctypes.data, 0) == -1
    assert L.sa_amd_index_set_documents(fake, offs.ctypes.data, -3) == -1
    assert L.sa_amd_index_set_documents(fake, np.array([1, 2, 4], dtype=np.uint32).ctypes.data, 2) == -1
    assert L.sa_amd_index_set_documents(fake, np.array([0, 5, 4], dtype=np.uint32).ctypes.data, 2) == -1
    assert L.sa_amd_index_doc_of(fake, p, -1, p) == -1                                          # negative count
    assert L.sa_amd_index_doc_of(fake, None, 4, p) == -1
    assert L.sa_amd_index_doc_of(fake, p, 4, None) == -1
    assert L.sa_amd_index_doc_of_device(fake, p, -1, p, None) == -1
    assert L.sa_amd_index_doc_of_device(fake, p + 2, 4, p, None) == -1                          # not 4-byte aligned
    assert L.sa_amd_index_doc_of_device(fake, p, 4, p + 1, None) == -1
    assert L.sa_amd_index_doc_search(fake, p, good.ctypes.data, -1, p, p) == -1
    assert L.sa_amd_index_doc_search(fake, p, None, 2, p, p) == -1
    assert L.sa_amd_index_doc_search(fake, None, good.ctypes.data, 2, p, p) == -1
    for off in bad:                                                                              # pat_off as sa_amd_index_search rejects it
        assert L.sa_amd_index_doc_search(fake, p, off.ctypes.data, 2, p, p) == -1
        assert L.sa_amd_index_doc_list(fake, p, off.ctypes.data, 2, p, p, 4, c) == -1
    assert L.sa_amd_index_doc_list(fake, p, good.ctypes.data, 2, p, p, -1, c) == -1             # negative capacity
    assert L.sa_amd_index_doc_list(fake, p, good.ctypes.data, 2, None, p, 4, c) == -1
    assert L.sa_amd_index_doc_list(fake, p, good.ctypes.data, 2, p, None, 4, c) == -1
    assert L.sa_amd_index_doc_list(fake, p, good.ctypes.data, 2, p, p, 4, None) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777)
    L.sa_amd_last_docs_stats(None)


def test_chunk_switch():
    try:
        assert sa.docs_set_chunk(100) == sa.DOC_CHUNK_DEFAULT
        assert sa.docs_set_chunk(0) == 100
        assert sa.docs_set_chunk(1 << 30) == sa.DOC_CHUNK_MIN
        assert sa.docs_set_chunk(-1) == sa.DOC_CHUNK_MAX
        assert sa.docs_set_chunk(-7) == sa.DOC_CHUNK_DEFAULT
    finally:
        sa.docs_set_chunk(-1)


@pytest.mark.parametrize("n", [0, 1, 4095, 1 << 20, 2**31 - 1])
def test_work_block(n):
    """control words, four (n + 1)-entry buffers, the sort's spine and granules: about 16 n"""
    w = sa.docs_work_bytes(n)
    assert w % 256 == 0 and 16 * (n + 1) <= w <= 17 * (n + 1) + (4 << 20)
