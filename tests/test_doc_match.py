"""GPU suite for Boolean document queries on the device index: doc_match and doc_match_list compared bit
for bit with the definitions of tests/test_doc_match_abi.py (Python sets over the oracle's suffix array, checked against brute force
there), their statistics with the model of the same file.

Sizes: the smallest at which each step can go wrong.  ndocs around one bitmap word, two words and one combine tile
(DOC_MATCH_TILE_WORDS words of 32 documents); texts of 0 bytes, 1 byte, 4 097 bytes and 1 MiB in 65 537 documents; ranges of one
slot fewer than, exactly, one more than a unit of 64 slots and one more than two; more units than one grid has waves; budgets
that give one slab, one query a slab and less than one query's bitmaps."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import Not, corpus
import dirty_blocks
import test_streams as streams
from test_docs_abi import EXAMPLE_OFF, EXAMPLE_TEXT, _u8, answers_definition
from test_doc_match_abi import BUDGET_MAX, BUDGET_MIN, match_definition, queries_of, stats_definition

pytestmark = pytest.mark.gpu

TILE_DOCS = sa.DOC_MATCH_TILE_WORDS * 32
_ACROSS_ROUTES = {}


def same_for_every_route(key, route, *arrays):
    """what the first route answered for `key` is what every other route answers, bit for bit (by digest)"""
    got = tuple(hashlib.sha256(np.asarray(a).astype(np.uint32).tobytes()).digest() for a in arrays)
    first = _ACROSS_ROUTES.setdefault(key, (route, got))
    assert first[1] == got, (key, "route", first[0], route)


def random_table(n, ndocs, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0], np.sort(rng.integers(0, n + 1, ndocs - 1)), [n]]).astype(np.int64)


def english(n, seed):
    t = corpus.english_corpus(n, seed)
    return t, t.tobytes()


def some_patterns(tb, seed, count=8):
    rng = np.random.default_rng(seed)
    n = len(tb)
    pats = [b"", b"\x01\x02nope"]
    for _ in range(count):
        a = int(rng.integers(0, max(n, 1)))
        pats.append(tb[a:a + int(rng.integers(1, 6))])
    return pats + [bytes([c]) for c in sorted(set(tb))[:3]]


def effective(chunk, budget):
    return (sa.DOC_CHUNK_DEFAULT if chunk < 0 else min(max(chunk, sa.DOC_CHUNK_MIN), sa.DOC_CHUNK_MAX),
            sa.DOC_MATCH_BUDGET_DEFAULT if budget < 0 else min(max(budget, BUDGET_MIN), BUDGET_MAX))


def check_match(ix, tb, off, arr, queries, chunk=-1, budget=-1, key=None, route=None):
    """doc_match with and without clause_df, doc_match_list and the statistics of each against the definitions"""
    df, cdf, lists = match_definition(tb, off, arr, queries)
    pc, pb = sa.docs_set_chunk(chunk), sa.doc_match_set_budget(budget)
    try:
        got_df, got_cdf = ix.doc_match(queries, clause_df=True)
        st = sa.last_doc_match_stats()
        only_df = ix.doc_match(queries)
        st1 = sa.last_doc_match_stats()
        got_lists = ix.doc_match_list(queries)
        st2 = sa.last_doc_match_stats()
    finally:
        sa.docs_set_chunk(pc)
        sa.doc_match_set_budget(pb)
    assert got_df.dtype == np.uint32 and np.array_equal(got_df, df), (got_df.tolist(), df.tolist())
    assert got_cdf.dtype == np.uint32 and np.array_equal(got_cdf, cdf)
    assert np.array_equal(only_df, df)                                # (the pass without the clause counts)
    assert len(got_lists) == len(queries)
    for q in range(len(queries)):
        assert got_lists[q].dtype == np.uint32 and np.array_equal(got_lists[q], lists[q]), q
    want = stats_definition(tb, off, arr, queries, *effective(chunk, budget), False)
    assert st == want and st1 == want, (st, st1, want)
    want.update(listed=1)
    if int(df.sum()) <= 1 << 16:                                      # (else DeviceIndex.doc_match_list has called twice: same numbers)
        assert st2 == want, (st2, want)
    if key is not None:
        flat = np.concatenate(list(got_lists) + [np.zeros(0, dtype=np.uint32)])
        same_for_every_route(key, route, got_df, got_cdf, flat)
    return df, cdf, lists


def raw_match(ix, queries, df=True, cdf=True):
    """sa_amd_index_doc_match on numpy buffers with canaries around both outputs -> (df, clause_df), None where not asked for"""
    data, off, npat, coff, cfl, ncl, qoff, nq = sa._query_batch(queries)
    a = np.full(nq + 32, 0xA5A5A5A5, dtype=np.uint32)
    b = np.full(ncl + 32, 0x5A5A5A5A, dtype=np.uint32)
    rc = sa.lib().sa_amd_index_doc_match(ix._h, data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl, qoff.ctypes.data,
                                         nq, a[16:].ctypes.data if df else None, b[16:].ctypes.data if cdf else None)
    assert rc == 0
    assert np.all(a[:16] == 0xA5A5A5A5) and np.all(a[16 + (nq if df else 0):] == 0xA5A5A5A5)
    assert np.all(b[:16] == 0x5A5A5A5A) and np.all(b[16 + (ncl if cdf else 0):] == 0x5A5A5A5A)
    return (a[16:16 + nq].copy() if df else None), (b[16:16 + ncl].copy() if cdf else None)


def raw_list(ix, queries, capacity):
    """sa_amd_index_doc_match_list with canaries around both outputs -> (total, list_off, the entries written)"""
    data, off, npat, coff, cfl, ncl, qoff, nq = sa._query_batch(queries)
    loff = np.full(nq + 1 + 16, -7, dtype=np.int64)
    docs = np.full(capacity + 64, 0xA5A5A5A5, dtype=np.uint32)
    total = ctypes.c_int64(-1)
    rc = sa.lib().sa_amd_index_doc_match_list(ix._h, data.ctypes.data, off.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl,
                                              qoff.ctypes.data, nq, loff[8:].ctypes.data, docs[32:].ctypes.data, capacity, ctypes.byref(total))
    assert rc == 0
    assert np.all(loff[:8] == -7) and np.all(loff[8 + nq + 1:] == -7)
    wrote = min(int(total.value), capacity)
    assert np.all(docs[:32] == 0xA5A5A5A5) and np.all(docs[32 + wrote:] == 0xA5A5A5A5)      # nothing before, nothing past what fits
    return int(total.value), loff[8:8 + nq + 1].copy(), docs[32:32 + wrote].astype(np.int64)


def test_known_answers(oracle):
    t = _u8(EXAMPLE_TEXT)
    ix = sa.DeviceIndex(t, oracle.sais(t))
    with pytest.raises(sa.SuffixArrayError):                          # a query before set_documents
        ix.doc_match([[b"a"]])
    with pytest.raises(sa.SuffixArrayError):
        ix.doc_match_list([[b"a"]])
    ix.set_documents(EXAMPLE_OFF)
    queries = [[b"a", b"bra"], [b"a", Not(b"bra")], [Not(b"a")], [[b"c", b"bra"]], [b"ac"], [b"a", b"c", b"bra"], []]
    df, cdf = ix.doc_match(queries, clause_df=True)
    assert df.tolist() == [2, 1, 1, 3, 1, 0, 4] and cdf.tolist() == [3, 2, 3, 2, 1, 3, 1, 3, 1, 2]
    assert [l.tolist() for l in ix.doc_match_list(queries)] == [[0, 3], [2], [1], [0, 2, 3], [0], [], [0, 1, 2, 3]]
    before = sa.last_doc_match_stats()
    assert ix.doc_match([]).size == 0 and ix.doc_match_list([]) == []          # nqueries == 0: at once
    st = sa.last_doc_match_stats()
    assert (st["queries"], st["slabs"], st["readbacks"], st["listed"], before["queries"]) == (0, 0, 0, 1, 7)
    check_match(ix, EXAMPLE_TEXT, EXAMPLE_OFF, oracle.sais(t), queries, chunk=64)
    ix.close()
    s = sa.SuffixArray(t)                                              # the same on the lazily made index
    s.set_documents(EXAMPLE_OFF)
    assert s.doc_match([[b"a", Not(b"bra")]]).tolist() == [1] and s.doc_match_list([[Not(b"a")], []])[1].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("ndocs", [1, 31, 32, 33, 63, 64, 65, TILE_DOCS - 1, TILE_DOCS, TILE_DOCS + 1, 2 * TILE_DOCS + 33])
def test_tail_and_word_boundaries(oracle, ndocs):
    """the all-negated query and the query without clauses are the two a missing mask of the last word breaks: both must count
    exactly ndocs.  From 8 191 documents on there are more documents than bytes: runs of empty documents."""
    t, tb = english(3000, 5)
    arr = oracle.sais(t)
    off = random_table(t.size, ndocs, ndocs)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    pats = some_patterns(tb, ndocs)
    queries = [[], [Not(b"\x01\x02nope")], [Not(b"\x01\x02nope"), Not(b"\xf7")], [Not(pats[2]), Not(pats[3])]] + queries_of(pats, np.random.default_rng(ndocs))
    df, cdf, lists = check_match(ix, tb, off, arr, queries, chunk=64)
    assert df[:3].tolist() == [ndocs] * 3 and cdf[:3].tolist() == [ndocs] * 3
    assert lists[0].tolist() == list(range(ndocs)) and lists[0][-1] == ndocs - 1
    ix.close()


@pytest.mark.parametrize("text", [b"", b"a", b"ab" * 2048 + b"c"], ids=["0", "1", "4097"])
def test_small_texts(oracle, text):
    t = _u8(text)
    n = t.size
    arr = oracle.sais(t)
    tables = [[0, n], [0, 0, n, n], list(range(n + 1)) if 0 < n < 100 else [0] * 3 + [n // 2] * 2 + [n] * 3, random_table(n, 70, 3)]
    for k, off in enumerate(tables):
        ix = sa.DeviceIndex(t, arr)
        ix.set_documents(off)
        pats = [b"", b"a", b"b", b"ab", b"ba", b"c", b"bc", b"zz"]
        check_match(ix, text, off, arr, queries_of(pats, np.random.default_rng(k)), chunk=64)
        ix.close()


class _Mid:
    """1 MiB of English-like text in 65 537 documents: ndocs above 65 536 and well above DOC_SAMPLES; the index is shared"""

    def __init__(self, oracle):
        self.t, self.tb = english(1 << 20, 11)
        self.arr = oracle.sais(self.t)
        self.off = random_table(self.t.size, 65537, 7)
        self.ix = sa.DeviceIndex(self.t, self.arr)
        self.ix.set_documents(self.off)


@pytest.fixture(scope="module")
def mid(oracle):
    m = _Mid(oracle)
    try:
        yield m
    finally:
        m.ix.close()


def test_one_mebibyte_in_65537_documents(mid):
    pats = some_patterns(mid.tb, 12, 12) + [b"e", b" ", b"th", b"the ", b"and"]
    queries = queries_of(pats, np.random.default_rng(3)) + [[b"e", b" "], [b"e", Not(b" ")], [Not(b"e"), Not(b" ")], [[b"th", b"and"], Not(b"the ")]]
    df, _, _ = check_match(mid.ix, mid.tb, mid.off, mid.arr, queries)
    assert df[0] == 65537 and 0 < df[-4] < 65537
    assert df[-4] + df[-3] == match_definition(mid.tb, mid.off, mid.arr, [[b"e"]])[0][0]          # (e AND x) + (e AND NOT x) = e
    check_match(mid.ix, mid.tb, mid.off, mid.arr, queries[-4:], chunk=64, budget=BUDGET_MIN)       # every query a slab of its own


def test_more_units_than_one_grid_has_waves(mid):
    """the empty pattern at 64 slots a unit is 16 385 units, one more than the 16 384 waves of the largest grid (16 workgroups of
    four waves on each of 256 compute units); three of them and a pattern of its own keep every wave going round"""
    queries = [[b"", b"e"], [Not(b"")], [[b"", b"\x01\x02nope"]]]
    check_match(mid.ix, mid.tb, mid.off, mid.arr, queries, chunk=64)
    st = sa.last_doc_match_stats()
    assert st["units"] > 3 * 16384 and st["chunk"] == 64


def test_more_queries_than_one_grid_has_waves(oracle):
    """40 000 queries of one tile each: more (query, tile) items than the 32 768 waves of the largest combine grid (32 workgroups
    of four waves on each of 256 compute units), a scan of several tiles for the listing, list_off from several workgroups"""
    t, tb = english(2000, 31)
    arr = oracle.sais(t)
    off = random_table(t.size, 70, 6)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    shapes = [[], [b"e"], [Not(b"e")], [b"e", b"t"], [[b"a", b"o"], Not(b"th")], [[]], [b"", Not(b"q")]]
    queries = [shapes[(k * k + k // 7) % len(shapes)] for k in range(40000)]
    df, _, _ = check_match(ix, tb, off, arr, queries, chunk=64)
    assert df.size == 40000 > 32768 and df[0] == 70
    check_match(ix, tb, off, arr, queries[:5000], budget=BUDGET_MIN)  # 8 bytes a clause: 512 clauses a slab
    assert sa.last_doc_match_stats()["slabs"] > 8
    ix.close()


def _chunk_text():
    """byte c occurs counts[c] times, so its range starts at slot 1 + the sum of the smaller bytes' counts: ranges of 63, 64, 65
    and 129 slots that begin on, and one off, a multiple of 64"""
    counts = {1: 63, 2: 64, 3: 65, 4: 129, 5: 63, 6: 0, 7: 320, 8: 1, 9: 127, 10: 64}
    t = np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in counts.items()])
    np.random.default_rng(13).shuffle(t)
    return t, counts


@pytest.mark.parametrize("chunk", [64, 100, 129, -1])
def test_units(oracle, chunk):
    t, counts = _chunk_text()
    tb = t.tobytes()
    arr = oracle.sais(t)
    off = random_table(t.size, 37, 8)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    singles = [bytes([b]) for b in counts]
    occ, _, _ = answers_definition(tb, off, arr, singles)
    assert occ.tolist() == list(counts.values()) and {63, 64, 65, 129} <= set(occ.tolist())
    queries = [[p] for p in singles] + [[Not(p)] for p in singles] + [[singles[k], Not(singles[k + 1])] for k in range(9)]
    queries += [[singles[:4]], [singles[4:], Not(singles[:2])], [b"", singles[6]], singles[:3]]
    check_match(ix, tb, off, arr, queries, chunk=chunk, key="units", route=chunk)
    ix.close()


def test_slabs(oracle):
    """40 000 documents are 1 250 words, 5 000 bytes of bitmap a clause.  Budgets: the default (one slab), exactly one two-clause
    query's bitmaps (one query a slab), and 4 KiB (less than one clause: still one query a slab)"""
    t, tb = english(6000, 21)
    arr = oracle.sais(t)
    ndocs = 40000
    off = random_table(t.size, ndocs, 4)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    pats = some_patterns(tb, 22)
    rng = np.random.default_rng(5)
    queries = [[pats[int(rng.integers(0, len(pats)))], Not(pats[int(rng.integers(0, len(pats)))])] for _ in range(6)]
    row = 4 * ((ndocs + 31) // 32)
    for budget, slabs in ((-1, 1), (6 * 2 * row, 1), (6 * 2 * row - 1, 2), (4 * row, 3), (2 * row, 6), (2 * row - 1, 6), (BUDGET_MIN, 6)):
        check_match(ix, tb, off, arr, queries, chunk=64, budget=budget, key="slabs", route=budget)
        assert sa.last_doc_match_stats()["slabs"] == slabs, budget
    mixed = [[], [pats[2]], [pats[3], pats[4], Not(pats[5])], [], [], [[pats[2], pats[3]]], [Not(pats[6])] * 5]
    for budget in (-1, 3 * row, BUDGET_MIN):
        check_match(ix, tb, off, arr, mixed, budget=budget, key="slabs_mixed", route=budget)
    ix.close()


@pytest.mark.parametrize("tables", [(), ("bkt",), ("lcp",), ("bkt", "lcp")], ids=["plain", "bkt", "lcp", "bkt_lcp"])
def test_answers_do_not_depend_on_the_route(oracle, tables):
    """one digest over chunk x budget x (LCP table on / off) x (bucket table on / off)"""
    t, tb = english(30000, 14)
    arr = oracle.sais(t)
    off = random_table(t.size, 9000, 9)                               # 282 words: 1 128 bytes a clause
    ix = sa.DeviceIndex(t, arr)
    if "bkt" in tables:
        ix.buckets()
    if "lcp" in tables:
        ix.enable_lcp()
    ix.set_documents(off)
    pats = some_patterns(tb, 15, 20) + [b"e", b"th", b"the ", b"zq", b"q\x00"]
    queries = queries_of(pats, np.random.default_rng(6))
    for chunk in (64, 77, -1):
        for budget in (BUDGET_MIN, 20000, -1):
            check_match(ix, tb, off, arr, queries, chunk=chunk, budget=budget, key="routes", route=(tables, chunk, budget))
    ix.close()


def test_outputs(oracle):
    t, tb = english(20000, 16)
    arr = oracle.sais(t)
    off = random_table(t.size, 300, 10)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    queries = [[b"e", b"th"], [b"\x01zq"], [Not(b"and")], [], [[b"the", b"of"], Not(b"q")]]
    df, cdf, lists = match_definition(tb, off, arr, queries)
    flat = np.concatenate(lists)
    total = int(df.sum())
    loff = np.concatenate([[0], np.cumsum(df)])
    middle = int(loff[2] + df[2] // 2)                                # inside the third query's listing
    assert df[2] >= 2 and df[1] == 0 and df[3] == 300 and total > middle
    for budget in (-1, BUDGET_MIN):
        prev = sa.doc_match_set_budget(budget)
        try:
            for capacity in (0, 1, middle, total - 1, total, total + 1000):
                got_total, got_loff, got = raw_list(ix, queries, capacity)
                assert got_total == total and np.array_equal(got_loff, loff)
                assert np.array_equal(got, flat[:min(capacity, total)])
                assert sa.last_doc_match_stats()["df_sum"] == total
            for want_df, want_cdf in ((True, True), (True, False), (False, True), (False, False)):
                got_df, got_cdf = raw_match(ix, queries, want_df, want_cdf)
                assert got_df is None or np.array_equal(got_df, df)
                assert got_cdf is None or np.array_equal(got_cdf, cdf)
                assert sa.last_doc_match_stats()["df_sum"] == total
        finally:
            sa.doc_match_set_budget(prev)
    L = sa.lib()
    data, poff, npat, coff, cfl, ncl, qoff, nq = sa._query_batch(queries)
    buf = np.full(16, 7, dtype=np.int64)
    tot = ctypes.c_int64(-3)
    args = (ix._h, data.ctypes.data, poff.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl, qoff.ctypes.data)
    assert L.sa_amd_index_doc_match_list(*args, nq, buf.ctypes.data, None, 5, ctypes.byref(tot)) == -1
    assert L.sa_amd_index_doc_match_list(*args, nq, buf.ctypes.data, buf.ctypes.data, -1, ctypes.byref(tot)) == -1
    assert tot.value == -3 and np.all(buf == 7)
    assert L.sa_amd_index_doc_match_list(*args, 0, buf.ctypes.data, None, 0, ctypes.byref(tot)) == -1      # query_off does not end at nclauses
    zero = np.zeros(1, dtype=np.int32)                                # nqueries == 0: list_off[0] = 0 and the total, nothing else
    assert L.sa_amd_index_doc_match_list(ix._h, None, None, 0, zero.ctypes.data, None, 0, zero.ctypes.data, 0, buf.ctypes.data, None, 0,
                                         ctypes.byref(tot)) == 0
    assert tot.value == 0 and buf.tolist() == [0] + [7] * 15
    assert L.sa_amd_index_doc_match(ix._h, None, None, 0, zero.ctypes.data, None, 0, zero.ctypes.data, 0, None, None) == 0
    one = np.array([0, 0], dtype=np.int32)                            # no pattern and no clause at all, one query: every document
    out = np.full(3, 9, dtype=np.uint32)
    assert L.sa_amd_index_doc_match(ix._h, None, None, 0, zero.ctypes.data, None, 0, one.ctypes.data, 1, out.ctypes.data, None) == 0
    assert out.tolist() == [300, 9, 9] and sa.last_doc_match_stats()["readbacks"] == 0
    ix.close()


def test_wrong_permutation_stays_in_bounds(oracle):
    """an array that is not the suffix array: the answers are unspecified, the calls succeed and every output stays inside its
    buffer and its value range"""
    t, tb = english(5000, 18)
    arr = np.random.default_rng(3).permutation(t.size + 1).astype(np.uint32)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(random_table(t.size, 64, 12))
    queries = queries_of(some_patterns(tb, 19) + [b"e", b" "], np.random.default_rng(7))
    prev = sa.docs_set_chunk(64)
    try:
        df, cdf = raw_match(ix, queries)
        assert np.all(df <= 64) and np.all(cdf <= 64)
        total, loff, docs = raw_list(ix, queries, 500)
        assert loff[0] == 0 and loff[-1] == total and np.all(np.diff(loff) >= 0) and np.all(docs < 64)
    finally:
        sa.docs_set_chunk(prev)
    ix.close()


def test_recycled_blocks(oracle):
    """the queries under the diagnostic library's fill of every pooled block, each pattern in turn: the answers are the model's
    and the statistics the clean run's.  A bitmap that is not zeroed in every call fails here."""
    t, tb = english(20000, 23)
    arr = oracle.sais(t)
    off = random_table(t.size, 9000, 2)
    pats = some_patterns(tb, 24)
    queries = queries_of(pats, np.random.default_rng(8))
    model = match_definition(tb, off, arr, queries)

    def run(ix):
        out = []
        for budget in (-1, BUDGET_MIN):
            prev = sa.doc_match_set_budget(budget)
            try:
                df, cdf = ix.doc_match(queries, clause_df=True)
                st = sa.last_doc_match_stats()
                lists = ix.doc_match_list(queries)
                st2 = sa.last_doc_match_stats()
            finally:
                sa.doc_match_set_budget(prev)
            assert np.array_equal(df, model[0]) and np.array_equal(cdf, model[1])
            assert all(np.array_equal(a, b) for a, b in zip(lists, model[2]))
            out += [st, st2]
        return out

    with dirty_blocks.diag_library() as d:
        assert d.fill(None) == dirty_blocks.FILL_OFF
        ix = d.index(t, arr)
        ix.set_documents(off)
        clean = run(ix)
        assert clean[0] == stats_definition(tb, off, arr, queries, sa.DOC_CHUNK_DEFAULT, sa.DOC_MATCH_BUDGET_DEFAULT, False)
        for pattern in dirty_blocks.ORDER:
            d.fill(pattern)
            try:
                got = run(ix)
            finally:
                assert d.fill(None) == dirty_blocks.PATTERNS[pattern]
            assert got == clean, pattern


def test_calls_neither_need_nor_disturb_a_busy_non_blocking_stream(oracle):
    """doc_match and doc_match_list while a caller's non-blocking stream is busy with unrelated copies (the delay chain of
    tests/test_streams.py): the calls answer without that stream having drained and its buffers come out untouched"""
    t, tb = english(20000, 25)
    arr = oracle.sais(t)
    off = random_table(t.size, 500, 3)
    queries = queries_of(some_patterns(tb, 26), np.random.default_rng(9))
    df, cdf, lists = match_definition(tb, off, arr, queries)
    env = streams.Env()
    hip = env.hip
    S = env.stream()
    ix = sa.DeviceIndex(t, arr)
    try:
        ix.set_documents(off)
        pattern = np.arange(streams.SCRATCH // 8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        assert hip.hipMemcpy(env.scratch[0], pattern.ctypes.data, streams.SCRATCH, streams.H2D) == 0
        assert hip.hipMemset(env.scratch[1], 0, streams.SCRATCH) == 0
        assert hip.hipDeviceSynchronize() == 0

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        got_df, got_cdf = ix.doc_match(queries, clause_df=True)
        assert np.array_equal(got_df, df) and np.array_equal(got_cdf, cdf)

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        got = ix.doc_match_list(queries)
        assert all(np.array_equal(a, b) for a, b in zip(got, lists))

        assert hip.hipStreamSynchronize(S) == 0
        back = np.empty_like(pattern)
        for p in env.scratch:                                         # an even number of copies each: both buffers hold the pattern
            assert hip.hipMemcpy(back.ctypes.data, p, streams.SCRATCH, streams.D2H) == 0
            assert np.array_equal(back, pattern)
    finally:
        hip.hipStreamSynchronize(S)
        hip.hipStreamDestroy(S)
        ix.close()
        env.close()


def test_threads_and_statistics(oracle):
    t, tb = english(40000, 17)
    arr = oracle.sais(t)
    off = random_table(t.size, 9000, 11)
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    ix.enable_doc_freq()
    pats = some_patterns(tb, 20, 12) + [b"e", b" "]
    # the other features' statistics are not touched by these calls, nor these by theirs
    ix.doc_search(pats)
    ix.doc_tf(pats)
    ix.next_bytes(pats)
    others = (sa.last_docs_stats(), sa.last_doc_tf_stats(), sa.last_ngram_stats())
    check_match(ix, tb, off, arr, queries_of(pats, np.random.default_rng(1)), chunk=64, budget=20000)
    assert (sa.last_docs_stats(), sa.last_doc_tf_stats(), sa.last_ngram_stats()) == others
    mine = sa.last_doc_match_stats()
    assert mine["listed"] == 1 and mine["readbacks"] == 1
    ix.doc_search(pats)
    ix.doc_list(pats)
    ix.doc_tf(pats)
    assert sa.last_doc_match_stats() == mine

    batches = [queries_of(some_patterns(tb, 30 + j, 12), np.random.default_rng(j)) for j in range(2)]
    exp = [match_definition(tb, off, arr, b) for b in batches]
    settings = [(500, 20000), (64, BUDGET_MIN)]
    errors = []

    def work(j):
        try:
            chunk, budget = settings[j]
            sa.docs_set_chunk(chunk)                                  # (the switches are the calling thread's)
            sa.doc_match_set_budget(budget)
            want = stats_definition(tb, off, arr, batches[j], chunk, budget, False)
            for _ in range(3):
                df, cdf = ix.doc_match(batches[j], clause_df=True)
                assert np.array_equal(df, exp[j][0]) and np.array_equal(cdf, exp[j][1])
                assert sa.last_doc_match_stats() == want
                lists = ix.doc_match_list(batches[j])
                assert all(np.array_equal(a, b) for a, b in zip(lists, exp[j][2]))
                assert sa.last_doc_match_stats()["budget"] == budget
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.doc_match_set_budget(-1) == sa.DOC_MATCH_BUDGET_DEFAULT  # the workers' switches were their own: this thread's is untouched
    assert sa.docs_set_chunk(-1) == sa.DOC_CHUNK_DEFAULT
    assert sa.last_doc_match_stats() == mine
    ix.close()


def test_agreement_with_doc_search_and_doc_list(oracle):
    """a query of one clause of one pattern: df is doc_search's, the listing is doc_list's, sorted"""
    t, tb = english(50000, 27)
    ix = sa.DeviceIndex(t, oracle.sais(t))
    ix.set_documents(random_table(t.size, 3000, 5))
    pats = some_patterns(tb, 28, 30) + [b"e", b" ", b"th"]
    _, df = ix.doc_search(pats)
    listed = ix.doc_list(pats)
    queries = [[p] for p in pats]
    got_df, got_cdf = ix.doc_match(queries, clause_df=True)
    assert np.array_equal(got_df, df) and np.array_equal(got_cdf, df)
    for a, b in zip(ix.doc_match_list(queries), listed):
        assert np.array_equal(a, np.sort(b))
    assert sa.last_doc_match_stats()["marks"] == int(df.sum()) == sa.last_doc_match_stats()["df_sum"]
    ix.close()
