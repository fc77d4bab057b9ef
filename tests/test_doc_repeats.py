"""GPU suite for document-aware duplicate spans over the device index: sa_amd_index_doc_repeat_spans compared bit for bit with
the definitions of tests/test_doc_repeats_abi.py (numpy over the oracle's suffix array, checked against the literal double loop
there): spans, doc_bytes and every statistic, for the four (mode, scope) pairs.

Sizes: texts from 0 bytes to 4 MiB + 6149, the smallest at which the kernels change their path (the edges of the tile of 2048
slots; a run through whole tiles without a head; more than 1024 tiles, where a thread of the spines owns more than one; more
tiles than the slot pass has workgroups).  The
range above 1 GiB is left to tests/test_top_of_range.py's conventions, as for the collections themselves: every position of these
kernels is below n + 1 < 2^31 and every sum with min_len is taken in 64 bits."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_docs_abi import EXAMPLE_OFF, EXAMPLE_TEXT
from test_doc_repeats_abi import ALL, ANY, COMBOS, KEEP_FIRST, OTHER, doc_repeats_definition, ks_of
from test_lcp_abi import _kasai
from test_repeats_abi import _u8, keep_first_definition, repeat_lengths_definition, spans_definition, stats_definition

pytestmark = pytest.mark.gpu

SPAN_CANARY, DOC_CANARY = 0xA5A5A5A5, 0x5A5A5A5A
TILE = 2048                                                           # REP_TILE of kernels/repeats.hpp


def raw(ix, k, mode, scope, capacity, ndocs, with_doc_bytes=True):
    """the C call on numpy buffers with canaries around both outputs -> (rc, count, the spans written, doc_bytes or None)"""
    spans = np.full(2 * capacity + 64, SPAN_CANARY, dtype=np.uint32)
    db = np.full(ndocs + 64, DOC_CANARY, dtype=np.uint32)
    count = ctypes.c_int64(-7)
    rc = sa.lib().sa_amd_index_doc_repeat_spans(ix._h, k, mode, scope, spans[32:].ctypes.data, capacity, ctypes.byref(count),
                                                db[32:].ctypes.data if with_doc_bytes else None)
    if rc != 0:
        assert count.value == -7 and np.all(spans == SPAN_CANARY) and np.all(db == DOC_CANARY)      # nothing written
        return rc, None, None, None
    wrote = min(int(count.value), capacity)
    assert np.all(spans[:32] == SPAN_CANARY) and np.all(spans[32 + 2 * wrote:] == SPAN_CANARY)      # nothing before, nothing past what fits
    assert np.all(db[:32] == DOC_CANARY) and np.all(db[32 + (ndocs if with_doc_bytes else 0):] == DOC_CANARY)
    return rc, int(count.value), spans[32:32 + 2 * wrote].reshape(-1, 2).astype(np.int64), db[32:32 + ndocs].astype(np.int64) if with_doc_bytes else None


class Case:
    """a text, its oracle arrays and an index over it"""

    def __init__(self, oracle, text):
        self.t = _u8(text)
        self.n = self.t.size
        self.arr = oracle.sais(self.t)
        self.lcp = _kasai(oracle, self.t, self.arr)
        self.lr = repeat_lengths_definition(self.t, self.arr, self.lcp)
        self.ix = sa.DeviceIndex(self.t, self.arr)
        self.off = None

    def documents(self, off):
        self.off = np.asarray(off, dtype=np.int64)
        self.ix.set_documents(self.off)
        return self

    def want(self, k, mode, scope):
        return doc_repeats_definition(self.t, self.off, self.arr, self.lcp, k, mode, scope)

    def check(self, k, combos=COMBOS):
        """spans, doc_bytes and statistics of every pair against the model; returns the model's answers"""
        ndocs = self.off.size - 1
        out = {}
        for mode, scope in combos:
            w = self.want(k, mode, scope)
            rc, count, spans, db = raw(self.ix, k, mode, scope, sa.repeat_spans_bound(self.n, k) + 1, ndocs)
            assert rc == 0
            st, rs = sa.last_doc_repeat_stats(), sa.last_repeat_stats()
            assert count == w["spans"].shape[0] and np.array_equal(spans, w["spans"]), (k, mode, scope)
            assert np.array_equal(db, w["doc_bytes"]), (k, mode, scope)
            readbacks = st.pop("readbacks")
            assert st == w["stats"], (k, mode, scope, st, w["stats"])
            assert readbacks == rs["readbacks"] >= (2 if self.n else 1)       # the range pass, (the front end's,) the counters
            assert (rs["spans"], rs["covered_bytes"], rs["flagged"]) == (st["spans"], st["covered_bytes"], st["flagged"])
            base = stats_definition(self.t, self.lcp, self.lr, w["spans"], w["flagged"])
            assert {f: rs[f] for f in ("longest", "longest_pos", "lcp_sum", "distinct_substrings")} == \
                   {f: base[f] for f in ("longest", "longest_pos", "lcp_sum", "distinct_substrings")}
            out[(mode, scope)] = w
        return out

    def close(self):
        self.ix.close()


def table(n, ndocs, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0], np.sort(rng.integers(0, n + 1, ndocs - 1)), [n]]).astype(np.int64)


def even_table(n, size):
    return np.concatenate([np.arange(0, n, size), [n]]).astype(np.int64)


def low_entropy(n, seed, sigma=3):
    return np.random.default_rng(seed).integers(97, 97 + sigma, n).astype(np.uint8)


def digest(*arrays):
    return tuple(hashlib.sha256(np.asarray(a).astype(np.int64).tobytes()).digest() for a in arrays)


def test_known_answers(oracle):
    c = Case(oracle, EXAMPLE_TEXT).documents(EXAMPLE_OFF)
    assert c.ix.doc_repeat_spans(1, sa.REPEATS_KEEP_FIRST, sa.DOCREP_ANY).tolist() == [[3, 4], [5, 6], [7, 11]]
    spans, db = c.ix.doc_repeat_spans(1, doc_bytes=True)              # the defaults: KEEP_FIRST, OTHER
    assert spans.dtype == np.uint32 and spans.tolist() == [[5, 6], [7, 11]] and db.dtype == np.uint32 and db.tolist() == [0, 0, 1, 4]
    assert sa.last_doc_repeat_stats() == {"members": 11, "flagged": 5, "spans": 2, "covered_bytes": 5, "docs_touched": 2,
                                          "readbacks": sa.last_repeat_stats()["readbacks"]}
    for scope in (sa.DOCREP_ANY, sa.DOCREP_OTHER):
        assert c.ix.doc_repeat_spans(3, sa.REPEATS_ALL, scope).tolist() == [[0, 4], [7, 11]]
    for k in (1, 2, 3, 4, 5):
        c.check(k)
    c.close()
    c = Case(oracle, b"aaaa").documents([0, 2, 4])
    assert c.ix.doc_repeat_spans(2).tolist() == [[2, 4]] and c.ix.repeat_spans(2, keep_first=True).tolist() == [[1, 4]]
    spans, db = c.ix.doc_repeat_spans(2, sa.REPEATS_ALL, sa.DOCREP_OTHER, doc_bytes=True)
    assert spans.tolist() == [[0, 4]] and db.tolist() == [2, 2]
    c.close()
    s = sa.SuffixArray(_u8(EXAMPLE_TEXT))                              # the same on the lazily made index
    s.set_documents(EXAMPLE_OFF)
    assert s.doc_repeat_spans(1, sa.REPEATS_KEEP_FIRST, sa.DOCREP_ANY).tolist() == [[3, 4], [5, 6], [7, 11]]
    assert s.doc_repeat_spans(1, doc_bytes=True)[1].tolist() == [0, 0, 1, 4]
    with pytest.raises(ValueError):
        s.doc_repeat_spans(0)


@pytest.mark.parametrize("n", [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_sizes_around_the_tile(oracle, n):
    c = Case(oracle, low_entropy(n, n + 3))
    for name, off in (("one", [0, n]), ("cuts", table(n, 9, n)), ("empties", [0, 0, n // 3, n // 3, n, n]), ("short", even_table(n, 5) if n else [0, 0])):
        c.documents(off)
        for k in ks_of(c.off, n):
            got = c.check(k)
            if len(off) == 2:                                         # one document: the identities of the header
                assert np.array_equal(got[(KEEP_FIRST, ANY)]["spans"], keep_first_definition(c.t, c.arr, c.lcp, k)[0])
                assert np.array_equal(got[(ALL, ANY)]["spans"], spans_definition(c.lr, k)[0])
                assert got[(ALL, OTHER)]["spans"].size == 0 and got[(KEEP_FIRST, OTHER)]["spans"].size == 0
    c.close()


def test_one_run_through_whole_tiles(oracle):
    """b"a" * 6145: for k = 3 every slot from 4 on has LCP >= 3 -- one run through three whole tiles without a head, so the spine's
    carry must pass through them; with 7-byte documents the members form a periodic pattern (5 of every 7 positions)"""
    n = 3 * TILE + 1
    c = Case(oracle, b"a" * n).documents(even_table(n, 7))
    got = c.check(3)
    assert got[(ALL, ANY)]["stats"]["members"] == 5 * (n // 7) + max(n % 7 - 2, 0)
    assert got[(KEEP_FIRST, OTHER)]["stats"]["flagged"] == got[(ALL, ANY)]["stats"]["members"] - 5
    for k in (1, 7, 8):
        c.check(k)
    c.documents(np.arange(n + 1))                                     # one-byte documents: only k = 1 has members
    got = c.check(1)
    assert got[(ALL, OTHER)]["stats"] == {"members": n, "flagged": n, "spans": 1, "covered_bytes": n, "docs_touched": n}
    assert got[(KEEP_FIRST, OTHER)]["stats"]["flagged"] == n - 1
    got = c.check(2)
    assert all(a["stats"]["members"] == 0 and a["spans"].size == 0 for a in got.values())
    c.close()


def test_period_two_across_tile_edges(oracle):
    n = 2 * TILE + 2
    c = Case(oracle, b"ab" * (n // 2))
    for off in (even_table(n, 2), even_table(n, 3), table(n, 40, 2), [0, TILE - 1, TILE, TILE + 1, 2 * TILE, n]):
        c.documents(off)
        for k in (1, 2, 3, 5, 600):
            c.check(k)
    c.close()


def test_more_than_1024_tiles_english_4k_documents(oracle):
    """2 Mi + 6149 bytes: 1028 tiles, so threads of the spines own more than one tile; English-like text in 4 KiB documents"""
    n = (2 << 20) + 6149
    c = Case(oracle, corpus.english_corpus(n, 21)).documents(even_table(n, 4096))
    got = c.check(12)
    assert got[(KEEP_FIRST, OTHER)]["stats"]["flagged"] > 1000 and got[(ALL, ANY)]["stats"]["docs_touched"] > 256
    c.documents([0, n])                                               # one document: sa_amd_index_repeat_spans' answers
    for mode in (ALL, KEEP_FIRST):
        rc, count, spans, db = raw(c.ix, 12, mode, ANY, sa.repeat_spans_bound(n, 12), 1)
        st = sa.last_doc_repeat_stats()
        blind = c.ix.repeat_spans(12, keep_first=mode == KEEP_FIRST).astype(np.int64)
        rs = sa.last_repeat_stats()
        assert rc == 0 and np.array_equal(spans, blind) and count == rs["spans"] == st["spans"]
        assert (st["flagged"], st["covered_bytes"]) == (rs["flagged"], rs["covered_bytes"]) and db.tolist() == [rs["covered_bytes"]]
        rc, count, spans, db = raw(c.ix, 12, mode, OTHER, 8, 1)
        assert rc == 0 and count == 0 and db.tolist() == [0] and sa.last_doc_repeat_stats()["flagged"] == 0
    c.close()


def test_more_tiles_than_resident_workgroups(oracle):
    """4 MiB + 6149 bytes: 2052 tiles, twice what the slot pass has workgroups on a device of 256 compute units (four a unit):
    every workgroup walks over more than one tile with the samples it staged once"""
    n = (4 << 20) + 6149
    c = Case(oracle, corpus.english_corpus(n, 22)).documents(even_table(n, 3000))
    got = c.check(16, [(KEEP_FIRST, OTHER), (ALL, ANY)])
    assert got[(KEEP_FIRST, OTHER)]["stats"]["flagged"] > 1000
    c.close()


def test_more_documents_than_bytes_and_than_65536(oracle):
    n = 5000
    c = Case(oracle, low_entropy(n, 9, 4)).documents(table(n, 70001, 4))
    assert c.off.size - 1 > 65536 > n
    for k in (1, 2, 3):
        got = c.check(k)
    assert got[(ALL, ANY)]["stats"]["members"] < n
    c.close()


def test_set_documents_again_changes_the_answers(oracle):
    n = 6000
    c = Case(oracle, low_entropy(n, 12)).documents(even_table(n, 64))
    a = c.check(8)
    c.documents(even_table(n, 11))
    b = c.check(8)
    assert a[(KEEP_FIRST, OTHER)]["stats"]["members"] != b[(KEEP_FIRST, OTHER)]["stats"]["members"]
    assert not np.array_equal(a[(KEEP_FIRST, OTHER)]["spans"], b[(KEEP_FIRST, OTHER)]["spans"])
    c.documents(even_table(n, 64))
    assert digest(c.check(8)[(ALL, OTHER)]["spans"]) == digest(a[(ALL, OTHER)]["spans"])
    c.close()


def test_same_answers_with_lcp_table_and_buckets(oracle):
    n = 30000
    c = Case(oracle, corpus.english_corpus(n, 4)).documents(table(n, 50, 1))
    seen = {}
    for route in ("plain", "buckets", "lcp"):
        if route == "buckets":
            c.ix.buckets()
        if route == "lcp":
            c.ix.enable_lcp()
        for mode, scope in COMBOS:
            rc, count, spans, db = raw(c.ix, 6, mode, scope, sa.repeat_spans_bound(n, 6), 50)
            assert rc == 0
            first = seen.setdefault((mode, scope), digest(spans, db, [count]))
            assert first == digest(spans, db, [count]), (route, mode, scope)
    c.check(6)
    c.close()


def test_capacities_and_doc_bytes_null(oracle):
    n = 20000
    c = Case(oracle, corpus.english_corpus(n, 6)).documents(even_table(n, 500))
    ndocs = c.off.size - 1
    for mode, scope in COMBOS:
        w = c.want(5, mode, scope)
        total = w["spans"].shape[0]
        assert total > 8
        for cap in (0, 1, total - 1, total, total + 1):
            rc, count, spans, db = raw(c.ix, 5, mode, scope, cap, ndocs)
            st = sa.last_doc_repeat_stats()
            assert rc == 0 and count == total and np.array_equal(spans, w["spans"][:cap]) and np.array_equal(db, w["doc_bytes"])
            st.pop("readbacks")
            assert st == w["stats"]                                   # the statistics cover all spans, written or not
            rc, count, spans2, none = raw(c.ix, 5, mode, scope, cap, ndocs, with_doc_bytes=False)
            st = sa.last_doc_repeat_stats()
            assert rc == 0 and count == total and np.array_equal(spans2, spans) and none is None
            assert st["docs_touched"] == -1 and st["covered_bytes"] == w["stats"]["covered_bytes"] and st["members"] == w["stats"]["members"]
    count = ctypes.c_int64(-1)                                        # capacity 0 takes a NULL spans
    assert sa.lib().sa_amd_index_doc_repeat_spans(c.ix._h, 5, ALL, ANY, None, 0, ctypes.byref(count), None) == 0
    assert count.value == c.want(5, ALL, ANY)["spans"].shape[0]
    c.close()


def test_readbacks_do_not_depend_on_the_data(oracle):
    n = 50000
    c = Case(oracle, corpus.english_corpus(n, 7)).documents(even_table(n, 1000))
    seen = set()
    for k in (2, 40):
        for mode, scope in COMBOS:
            for with_db in (True, False):
                assert raw(c.ix, k, mode, scope, 16, c.off.size - 1, with_db)[0] == 0
                seen.add(sa.last_doc_repeat_stats()["readbacks"])
    assert len(seen) == 1
    c.close()


def test_two_threads_query_one_index(oracle):
    n = 100000
    c = Case(oracle, corpus.english_corpus(n, 8)).documents(even_table(n, 777))
    ndocs = c.off.size - 1
    plans = [(6, KEEP_FIRST, OTHER), (9, ALL, ANY)]
    wants = [c.want(*p) for p in plans]
    errors = []

    def work(j):
        try:
            for _ in range(4):
                rc, count, spans, db = raw(c.ix, *plans[j], sa.repeat_spans_bound(n, plans[j][0]), ndocs)
                st = sa.last_doc_repeat_stats()
                st.pop("readbacks")
                assert rc == 0 and np.array_equal(spans, wants[j]["spans"]) and np.array_equal(db, wants[j]["doc_bytes"])
                assert st == wants[j]["stats"]
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    c.close()


def test_errors(oracle):
    t = _u8(b"mississippi")
    n = t.size
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    assert raw(ix, 2, ALL, ANY, 4, 2)[0] == -1                        # no collection set
    with pytest.raises(sa.SuffixArrayError):
        ix.doc_repeat_spans(2)
    ix.set_documents([0, 4, n])
    for k, mode, scope, cap in ((0, ALL, ANY, 4), (-3, ALL, ANY, 4), (2, 2, ANY, 4), (2, -1, ANY, 4), (2, ALL, 2, 4), (2, ALL, -1, 4),
                                (2, KEEP_FIRST, OTHER, -1)):
        assert raw(ix, k, mode, scope, cap, 2)[0] == -1, (k, mode, scope, cap)
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    cnt = ctypes.c_int64(-5)
    assert L.sa_amd_index_doc_repeat_spans(ix._h, 2, ALL, ANY, buf.ctypes.data, 4, None, buf[32:].ctypes.data) == -1      # NULL count_out
    assert L.sa_amd_index_doc_repeat_spans(ix._h, 2, ALL, ANY, None, 4, ctypes.byref(cnt), buf[32:].ctypes.data) == -1   # capacity > 0, NULL spans
    assert L.sa_amd_index_doc_repeat_spans(None, 2, ALL, ANY, buf.ctypes.data, 4, ctypes.byref(cnt), buf[32:].ctypes.data) == -1
    assert cnt.value == -5 and np.all(buf == 0x77777777)
    assert raw(ix, 2, ALL, ANY, 4, 2)[0] == 0                         # and the index still answers
    ix.close()
    bad = arr.copy()                                                  # the array's range errors, as for sa_amd_index_repeat_spans
    bad[5] = n + 1
    ix = sa.DeviceIndex(t, bad)
    ix.set_documents([0, n])
    assert raw(ix, 2, ALL, ANY, 4, 1)[0] == -6
    with pytest.raises(IndexError):
        ix.doc_repeat_spans(2)
    ix.close()
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]
    ix = sa.DeviceIndex(t, bad)
    ix.set_documents([0, n])
    assert raw(ix, 2, KEEP_FIRST, OTHER, 4, 1)[0] == -1
    ix.close()
    e = sa.DeviceIndex(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint32))       # the empty text in three empty documents
    e.set_documents([0, 0, 0, 0])
    rc, count, spans, db = raw(e, 1, ALL, ANY, 4, 3)
    assert rc == 0 and count == 0 and spans.size == 0 and db.tolist() == [0, 0, 0]
    assert sa.last_doc_repeat_stats()["members"] == 0 and sa.last_doc_repeat_stats()["docs_touched"] == 0
    e.close()


def test_wrong_permutation_stays_in_bounds():
    """unspecified answers, but the outputs' canaries hold, every span lies inside the text and doc_bytes sums to the covered bytes"""
    rng = np.random.default_rng(78)
    n = 50000
    t = corpus.english_corpus(n, 2)
    arr = np.empty(n + 1, dtype=np.uint32)
    arr[0] = n
    arr[1:] = rng.integers(0, n, n)                                   # in range, SA[0] = n, far from a permutation
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(even_table(n, 300))
    for mode, scope in COMBOS:
        rc, count, spans, db = raw(ix, 3, mode, scope, sa.repeat_spans_bound(n, 3), len(even_table(n, 300)) - 1)
        assert rc == 0 and np.all(spans[:, 0] < spans[:, 1]) and np.all(spans[:, 1] <= n)
        assert int(db.sum()) == sa.last_doc_repeat_stats()["covered_bytes"] == int(np.sum(spans[:, 1] - spans[:, 0]))
    ix.close()


def test_profile_classes_are_the_repeat_finders():
    L = sa.lib()
    names = []
    while True:
        nm = L.sa_amd_profile_kernel_name(len(names)).decode()
        if not nm:
            break
        names.append(nm)
    t = corpus.english_corpus(1 << 18, 8)
    ix = sa.DeviceIndex(t)
    ix.set_documents(even_table(t.size, 4096))
    L.sa_amd_profile_begin()
    ix.doc_repeat_spans(20, doc_bytes=True)
    cap = 32
    ms, launches, units = (ctypes.c_double * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
    cnt = L.sa_amd_profile_end(ms, launches, units, cap)
    got = {names[i]: launches[i] for i in range(cnt)}
    assert got["k_rep_lr"] == 3 and got["k_rep_spans"] == 6 and got["k_lcp_irreducible"] > 0, got
    ix.close()
