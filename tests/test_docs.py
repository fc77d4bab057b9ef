"""GPU suite for document collections over the device index: set_documents, doc_of, doc_search and doc_list compared bit for
bit with the definitions of tests/test_docs_abi.py (numpy over the oracle's suffix array, checked against brute force there).

Sizes: texts from 0 bytes to 1 MiB.  The range above 1 GiB is left to tests/test_top_of_range.py's conventions: the collection's
build needs the suffix array of such a text and 16 bytes of scratch per byte on top, which does not fit a few seconds here; every
index of these kernels is 64-bit or bounded by n + 1 < 2^31."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_lcp import _Dev
from test_docs_abi import (EXAMPLE_OFF, EXAMPLE_TEXT, NONE, _u8, answers_definition, doc_of_definition, units_definition,
                           word_definition)

pytestmark = pytest.mark.gpu

S = sa.DOC_SAMPLES
CANARY = 0xA5
_ACROSS_ROUTES = {}


def same_for_every_route(key, route, *arrays):
    """what the first route answered for `key` is what every other route answers, bit for bit (by digest)"""
    got = tuple(hashlib.sha256(np.asarray(a).astype(np.uint32).tobytes()).digest() for a in arrays)
    first = _ACROSS_ROUTES.setdefault(key, (route, got))
    assert first[1] == got, (key, "route", first[0], route)


def random_table(n, ndocs, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0], np.sort(rng.integers(0, n + 1, ndocs - 1)), [n]]).astype(np.int64)


def raw_list(ix, pats, capacity):
    """sa_amd_index_doc_list on numpy buffers with canaries around both outputs -> (total, list_off, the entries written)"""
    data, off, cnt = sa._pattern_batch(pats)
    loff = np.full(cnt + 1 + 16, -7, dtype=np.int64)
    docs = np.full(capacity + 64, 0xA5A5A5A5, dtype=np.uint32)
    total = ctypes.c_int64(-1)
    rc = sa.lib().sa_amd_index_doc_list(ix._h, data.ctypes.data, off.ctypes.data, cnt, loff[8:].ctypes.data, docs[32:].ctypes.data, capacity,
                                        ctypes.byref(total))
    assert rc == 0
    assert np.all(loff[:8] == -7) and np.all(loff[8 + cnt + 1:] == -7)
    wrote = min(int(total.value), capacity)
    assert np.all(docs[:32] == 0xA5A5A5A5) and np.all(docs[32 + wrote:] == 0xA5A5A5A5)      # nothing before, nothing past what fits
    return int(total.value), loff[8:8 + cnt + 1].copy(), docs[32:32 + wrote].astype(np.int64)


def check_queries(ix, tb, off, arr, pats, chunk=-1, key=None, route=None):
    """doc_search, doc_list and their statistics against the definitions; returns (occ, df, lists) of the model"""
    occ, df, lists = answers_definition(tb, off, arr, pats)
    prev = sa.docs_set_chunk(chunk)
    try:
        got_occ, got_df = ix.doc_search(pats)
        st = sa.last_docs_stats()
        got_lists = ix.doc_list(pats)
        st2 = sa.last_docs_stats()
    finally:
        sa.docs_set_chunk(prev)
    assert np.array_equal(got_occ, occ) and np.array_equal(got_df, df)
    assert len(got_lists) == len(pats)
    for q in range(len(pats)):
        assert got_lists[q].dtype == np.uint32 and np.array_equal(got_lists[q], lists[q]), (q, pats[q][:16])
        assert np.unique(got_lists[q]).size == got_lists[q].size == got_df[q]
    assert np.all(got_df <= np.minimum(got_occ, len(off) - 1))
    eff = sa.DOC_CHUNK_DEFAULT if chunk < 0 else min(max(chunk, sa.DOC_CHUNK_MIN), sa.DOC_CHUNK_MAX)
    want = {"patterns": len(pats), "occ_sum": int(occ.sum()), "units": units_definition(occ, eff), "df_sum": int(df.sum()),
            "slots_scanned": int(occ.sum()), "chunk": eff, "readbacks": 1 if pats else 0, "listed": 0}
    assert st == want, (st, want)
    want.update(slots_scanned=2 * int(occ.sum()), listed=1)
    if int(df.sum()) <= 1 << 16:                                      # (else DeviceIndex.doc_list has called twice: same numbers)
        assert st2 == want, (st2, want)
    if key is not None:
        flat = np.concatenate([l for l in got_lists] + [np.zeros(0, dtype=np.uint32)])
        same_for_every_route(key, route, got_occ, got_df, flat)
    return occ, df, lists


def check_doc_of(ix, off, n, extra=()):
    pos = np.concatenate([np.arange(min(n, 70000) + 3), np.asarray(extra, dtype=np.int64), [max(n - 1, 0), n, n + 1, NONE, NONE - 1]])
    got = ix.doc_of(pos.astype(np.uint32))
    assert got.dtype == np.uint32 and np.array_equal(got, doc_of_definition(off, n, pos))


def english(n, seed):
    t = corpus.english_corpus(n, seed)
    return t, t.tobytes()


def some_patterns(tb, seed, count=10):
    rng = np.random.default_rng(seed)
    n = len(tb)
    pats = [b"", b"\x01\x02nope", b"\xff"]
    for _ in range(count):
        a = int(rng.integers(0, max(n, 1)))
        pats.append(tb[a:a + int(rng.integers(1, 9))])
    if n > 64:
        pats.append(tb[n // 3:n // 3 + 60])                           # (long enough to occur once)
    return pats + [bytes([c]) for c in sorted(set(tb))[:3]]


def test_known_answers(oracle):
    t = _u8(EXAMPLE_TEXT)
    ix = sa.DeviceIndex(t, oracle.sais(t))
    ix.set_documents(EXAMPLE_OFF)
    occ, df = ix.doc_search([b"a", b"bra", b"", b"cad", b"zz"])
    assert occ.tolist() == [5, 2, 12, 1, 0] and df.tolist() == [3, 2, 3, 1, 0]
    assert [l.tolist() for l in ix.doc_list([b"a", b"bra", b"", b"zz"])] == [[3, 0, 2], [3, 0], [3, 0, 2], []]
    assert ix.doc_of([0, 3, 4, 6, 7, 10, 11, NONE]).tolist() == [0, 0, 2, 2, 3, 3, NONE, NONE]
    assert ix.doc_search([])[0].size == 0 and ix.doc_list([]) == []
    ix.close()
    s = sa.SuffixArray(t)                                              # the same four on the lazily made index
    s.set_documents(EXAMPLE_OFF)
    assert s.doc_search([b"a"])[1].tolist() == [3] and s.doc_list([b"bra"])[0].tolist() == [3, 0] and s.doc_of([5]).tolist() == [2]


@pytest.mark.parametrize("ndocs", [1, 2, S - 1, S, S + 1, 3 * S + 5])
def test_collections_around_the_sample_count(oracle, ndocs):
    t, tb = english(20000, 5)
    arr = oracle.sais(t)
    off = random_table(t.size, ndocs, ndocs)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    check_doc_of(ix, off, t.size, extra=off[off < t.size])
    check_queries(ix, tb, off, arr, some_patterns(tb, ndocs))
    ix.close()


def test_more_than_65536_documents_take_three_digit_passes(oracle):
    t, tb = english(300000, 6)
    arr = oracle.sais(t)
    off = random_table(t.size, 70001, 3)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    check_doc_of(ix, off, t.size, extra=np.arange(t.size - 70000, t.size))
    check_queries(ix, tb, off, arr, some_patterns(tb, 8) + [b"e", b"th", b" "])
    ix.close()


@pytest.mark.parametrize("shape", ["every_byte", "more_docs_than_bytes", "empty_first_last_runs"])
def test_many_and_empty_documents(oracle, shape):
    t, tb = english(3000, 7)
    n = t.size
    arr = oracle.sais(t)
    if shape == "every_byte":
        off = np.arange(n + 1)
    elif shape == "more_docs_than_bytes":
        off = random_table(n, 3 * n + 7, 4)
    else:
        off = np.concatenate([[0] * 40, random_table(n, 9, 5).repeat(3), [n] * 50])
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    check_doc_of(ix, off, n)
    occ, df, _ = check_queries(ix, tb, off, arr, some_patterns(tb, 9))
    assert df[0] == np.count_nonzero(np.diff(off)) and occ[0] == n + 1
    ix.close()


@pytest.mark.parametrize("ndocs", [1, 5])
def test_empty_text(oracle, ndocs):
    t = np.zeros(0, dtype=np.uint8)
    ix = sa.DeviceIndex(t, oracle.sais(t))
    ix.set_documents([0] * (ndocs + 1))
    assert ix.doc_of([0, 1, NONE]).tolist() == [NONE] * 3
    occ, df = ix.doc_search([b"", b"a"])
    assert occ.tolist() == [1, 0] and df.tolist() == [0, 0]
    assert [l.size for l in ix.doc_list([b"", b"a"])] == [0, 0]
    ix.close()


def test_tiny_texts(oracle):
    for b in (b"a", b"ab", b"aa", b"aba"):
        t = _u8(b)
        arr = oracle.sais(t)
        for off in ([0, len(b)], list(range(len(b) + 1)), [0, 0, 1, len(b), len(b)]):
            ix = sa.DeviceIndex(t, arr)
            ix.set_documents(off)
            check_doc_of(ix, off, t.size)
            check_queries(ix, b, off, arr, [b"", b"a", b"b", b"ab", b"ba", b"c"], chunk=64)
            ix.close()


def test_doc_of_on_device_pointers(oracle):
    """a position array that starts 4 bytes into its allocation, 256 canary bytes on either side of the output"""
    t, tb = english(50000, 8)
    off = random_table(t.size, 700, 6)
    ix = sa.DeviceIndex(t, oracle.sais(t))
    ix.set_documents(off)
    rng = np.random.default_rng(2)
    for count in (0, 1, 255, 2049, 40001):
        pos = rng.integers(0, t.size + 50, count).astype(np.uint32)
        pos[:count // 2:7] = NONE
        with _Dev(4 * count + 16, 4 * count + 512) as d:
            dP, dO = d.p
            assert d.hip.hipMemset(dO, CANARY, 4 * count + 512) == 0
            if count:
                assert d.hip.hipMemcpy(dP + 4, pos.ctypes.data, 4 * count, 1) == 0
            sa.doc_of_device_ptr(ix, dP + 4, count, dO + 256)
            raw = np.zeros(4 * count + 512, dtype=np.uint8)
            assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
            assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 4 * count:] == CANARY)
            assert np.array_equal(raw[256:256 + 4 * count].view(np.uint32), doc_of_definition(off, t.size, pos.astype(np.int64)))
            if count:
                with pytest.raises(sa.SuffixArrayError):
                    sa.doc_of_device_ptr(ix, dP + 2, count, dO + 256)      # not 4-byte aligned: nothing written
                assert d.hip.hipMemcpy(raw.ctypes.data, dO, 256, 2) == 0 and np.all(raw[:256] == CANARY)
    ix.close()


def test_replacing_a_collection_and_a_failed_replacement(oracle):
    t, tb = english(9000, 9)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    pats = some_patterns(tb, 10)
    for call in (lambda: ix.doc_of([1]), lambda: ix.doc_search(pats), lambda: ix.doc_list(pats)):
        with pytest.raises(sa.SuffixArrayError):                      # a query before set_documents
            call()
    first, second = random_table(t.size, 40, 1), random_table(t.size, 2000, 2)
    ix.set_documents(first)
    check_queries(ix, tb, first, arr, pats)
    for bad in ([0, 10, 5, t.size], [1, t.size], [0, t.size - 1], [0, t.size + 1], [0], []):
        with pytest.raises(sa.SuffixArrayError):
            ix.set_documents(bad)
        check_doc_of(ix, first, t.size)                                # the old one still answers
    check_queries(ix, tb, first, arr, pats)
    ix.set_documents(second)
    check_doc_of(ix, second, t.size)
    check_queries(ix, tb, second, arr, pats)
    ix.close()


def _mid():
    """1 MiB of English-like text with one document of a byte that occurs nowhere else"""
    t = corpus.english_corpus(1 << 20, 11).copy()
    assert 0xFE not in np.unique(t)
    t[500000:500100] = 0xFE
    off = np.unique(np.concatenate([random_table(t.size, 4096, 7), [500000, 500100]]))
    return t, off


def test_one_mebibyte(oracle):
    t, off = _mid()
    tb = t.tobytes()
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    check_doc_of(ix, off, t.size, extra=np.arange(t.size - 3000, t.size))
    pats = some_patterns(tb, 12, 20) + [b"e", b" ", b"t", b"a", b"\xfe", b"\xfe\xfe", b"\xfe" * 100, b"\xfe" * 101]
    occ, df, lists = check_queries(ix, tb, off, arr, pats)
    assert occ[pats.index(b"e")] > 10**4 and occ[pats.index(b" ")] > 10**5
    q = pats.index(b"\xfe")                                           # the range is all of one document's suffixes
    assert occ[q] == 100 and df[q] == 1 and lists[q].tolist() == [int(np.searchsorted(off, 500000))]
    assert np.count_nonzero(occ == 1) >= 1 and np.count_nonzero(occ == 0) >= 2
    # the documents of the matches of a query: POS of match_stats passed straight in
    query = np.concatenate([t[1000:1400], np.frombuffer(b"\x01\x02\x03", dtype=np.uint8), t[900000:900300]])
    ml, pos = ix.match_stats(query, 32)
    assert np.array_equal(ix.doc_of(pos), doc_of_definition(off, t.size, pos.astype(np.int64)))
    assert np.all(ix.doc_of(pos)[ml == 0] == NONE) and np.count_nonzero(ml == 0) >= 3
    # the stored word is the definition's: df of every range is one compare per slot
    w = word_definition(off, t.size, arr)
    lo = int(np.searchsorted(np.frombuffer(tb, dtype=np.uint8)[arr[1:]], ord("e"))) + 1
    assert ix.doc_search([b"e"])[1][0] == np.count_nonzero(w[lo:lo + occ[pats.index(b"e")]] <= lo)
    ix.close()


def _chunk_text():
    """byte c occurs counts[c] times, so its range starts at slot 1 + sum of the smaller bytes' counts: for chunk 64 the ranges
    have chunk - 1, chunk, chunk + 1 and 3 chunk + 1 slots and begin on, and one off, a multiple of chunk"""
    counts = {1: 63, 2: 64, 3: 65, 4: 193, 5: 63, 6: 0, 7: 320, 8: 1, 9: 127, 10: 64}
    t = np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in counts.items()])
    np.random.default_rng(13).shuffle(t)
    return t, counts


@pytest.mark.parametrize("chunk", [sa.DOC_CHUNK_MIN, 100, 193, sa.DOC_CHUNK_DEFAULT, 0, 1 << 30])
def test_chunk_sizes(oracle, chunk):
    t, counts = _chunk_text()
    tb = t.tobytes()
    arr = oracle.sais(t)
    off = random_table(t.size, 37, 8)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    singles = [bytes([b]) for b in counts]
    pats = []
    for p in singles:                                                  # many units per pattern beside zero units per pattern
        pats += [p, b"\xf0", p + b"\xf1", b""]
    occ, df, _ = answers_definition(tb, off, arr, singles)
    assert occ.tolist() == list(counts.values())
    starts = 1 + np.concatenate([[0], np.cumsum(occ)[:-1]])
    c0 = sa.DOC_CHUNK_MIN
    assert {c0 - 1, c0, c0 + 1, 3 * c0 + 1} <= set(occ.tolist())
    assert np.any((starts % c0 == 0) & (occ > 0)) and np.any((starts % c0 == 1) & (occ > 0))
    check_queries(ix, tb, off, arr, pats, chunk=chunk, key="chunks", route=chunk)
    check_queries(ix, tb, off, arr, singles, chunk=chunk)
    ix.close()


@pytest.mark.parametrize("tables", [(), ("bkt",), ("lcp",), ("bkt", "lcp")], ids=["plain", "bkt", "lcp", "bkt_lcp"])
def test_answers_do_not_depend_on_the_route(oracle, tables):
    t, tb = english(30000, 14)
    arr = oracle.sais(t)
    off = random_table(t.size, 500, 9)
    ix = sa.DeviceIndex(t, arr)
    if "bkt" in tables:
        ix.buckets()
    if "lcp" in tables:
        ix.enable_lcp()
    ix.set_documents(off)
    pats = some_patterns(tb, 15, 30) + [b"e", b"th", b"the ", b"zq", b"q\x00"]
    for chunk in (sa.DOC_CHUNK_MIN, 77, 4096, -1):
        check_queries(ix, tb, off, arr, pats, chunk=chunk, key="routes", route=(tables, chunk))
    ix.close()


def test_listing_capacity(oracle):
    t, tb = english(20000, 16)
    arr = oracle.sais(t)
    off = random_table(t.size, 300, 10)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    pats = [b"e", b"zq", b"th", b"", b"and"]
    occ, df, lists = answers_definition(tb, off, arr, pats)
    flat = np.concatenate(lists)
    total = int(df.sum())
    loff = np.concatenate([[0], np.cumsum(df)])
    middle = int(loff[2] + df[2] // 2)                                # inside the third pattern's listing
    assert df[2] >= 2 and total > middle
    prev = sa.docs_set_chunk(64)
    try:
        for capacity in (0, 1, middle, total - 1, total, total + 1000):
            got_total, got_loff, got = raw_list(ix, pats, capacity)
            assert got_total == total and np.array_equal(got_loff, loff)
            assert np.array_equal(got, flat[:min(capacity, total)])
            assert sa.last_docs_stats()["df_sum"] == total
    finally:
        sa.docs_set_chunk(prev)
    L = sa.lib()
    data, poff, cnt = sa._pattern_batch(pats)
    buf = np.full(16, 7, dtype=np.int64)
    tot = ctypes.c_int64(-3)
    assert L.sa_amd_index_doc_list(ix._h, data.ctypes.data, poff.ctypes.data, cnt, buf.ctypes.data, None, 5, ctypes.byref(tot)) == -1
    assert L.sa_amd_index_doc_list(ix._h, data.ctypes.data, poff.ctypes.data, cnt, buf.ctypes.data, None, -1, ctypes.byref(tot)) == -1
    assert tot.value == -3 and np.all(buf == 7)
    occ_only = np.zeros(cnt, dtype=np.uint32)                         # either output of doc_search may be NULL
    assert L.sa_amd_index_doc_search(ix._h, data.ctypes.data, poff.ctypes.data, cnt, occ_only.ctypes.data, None) == 0
    assert np.array_equal(occ_only, occ)
    assert L.sa_amd_index_doc_search(ix._h, data.ctypes.data, poff.ctypes.data, cnt, None, occ_only.ctypes.data) == 0
    assert np.array_equal(occ_only, df)
    ix.close()


def test_wrong_permutation_stays_in_bounds(oracle):
    """an array that is not the suffix array: the answers are unspecified, the calls succeed and every output stays inside its
    buffer and its value range"""
    t, tb = english(5000, 18)
    rng = np.random.default_rng(3)
    arr = rng.permutation(t.size + 1).astype(np.uint32)
    off = random_table(t.size, 64, 12)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    pats = some_patterns(tb, 19) + [b"e", b" "]
    prev = sa.docs_set_chunk(64)
    try:
        occ, df = ix.doc_search(pats)
        assert np.all(occ <= t.size + 1) and np.all(df <= occ)
        total, loff, docs = raw_list(ix, pats, 3000)
        assert loff[0] == 0 and loff[-1] == total and np.all(np.diff(loff) >= 0)
        assert np.all((docs < 64) | (docs == NONE))
        got = ix.doc_of(arr)
        assert np.array_equal(got, doc_of_definition(off, t.size, arr.astype(np.int64)))
    finally:
        sa.docs_set_chunk(prev)
    ix.close()


def test_two_threads_query_one_index(oracle):
    t, tb = english(40000, 17)
    arr = oracle.sais(t)
    off = random_table(t.size, 900, 11)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    batches = [some_patterns(tb, 20 + j, 25) + [b"e", b" "] for j in range(2)]
    exp = [answers_definition(tb, off, arr, b) for b in batches]
    errors = []

    def work(j):
        try:
            sa.docs_set_chunk(64 if j else 500)                       # (the switch is the calling thread's)
            for _ in range(4):
                occ, df = ix.doc_search(batches[j])
                assert np.array_equal(occ, exp[j][0]) and np.array_equal(df, exp[j][1])
                assert sa.last_docs_stats()["chunk"] == (64 if j else 500)
                lists = ix.doc_list(batches[j])
                assert all(np.array_equal(a, b) for a, b in zip(lists, exp[j][2]))
                assert np.array_equal(ix.doc_of(arr[:500]), doc_of_definition(off, t.size, arr[:500].astype(np.int64)))
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.docs_set_chunk(-1) == sa.DOC_CHUNK_DEFAULT              # the workers' switches were their own: this thread's is untouched
    ix.close()
