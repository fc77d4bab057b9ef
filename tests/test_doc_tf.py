"""GPU suite for per-document term frequencies and top-k documents over the device index: enable_doc_freq, doc_tf and doc_topk
compared bit for bit with the definitions of tests/test_doc_tf_abi.py (numpy over the oracle's suffix array, checked against
brute force there), the statistics with that file's model of the reduction.

Sizes: texts from 0 bytes to 1 MiB; every index of these kernels is 64-bit or bounded by n + 1 < 2^31."""
import ctypes
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_docs import english, random_table, raw_list, same_for_every_route, some_patterns
from test_docs_abi import EXAMPLE_OFF, EXAMPLE_TEXT, _u8
from test_doc_tf_abi import answers_definition, effective_piece, plan_definition, topk_definition

pytestmark = pytest.mark.gpu

S = sa.DOC_SAMPLES
FILL32 = 0xA5A5A5A5


def raw_tf(ix, pats, capacity, want_docs=True, want_tf=True):
    """sa_amd_index_doc_tf on numpy buffers with canaries around all three outputs -> (total, list_off, docs, tf) (what was written)"""
    data, off, cnt = sa._pattern_batch(pats)
    loff = np.full(cnt + 1 + 16, -7, dtype=np.int64)
    docs = np.full(capacity + 64, FILL32, dtype=np.uint32)
    tf = np.full(capacity + 64, FILL32, dtype=np.uint32)
    total = ctypes.c_int64(-1)
    rc = sa.lib().sa_amd_index_doc_tf(ix._h, data.ctypes.data, off.ctypes.data, cnt, loff[8:].ctypes.data, docs[32:].ctypes.data if want_docs else None,
                                      tf[32:].ctypes.data if want_tf else None, capacity, ctypes.byref(total))
    assert rc == 0
    assert np.all(loff[:8] == -7) and np.all(loff[8 + cnt + 1:] == -7)
    wrote = min(int(total.value), capacity)
    for buf, want in ((docs, want_docs), (tf, want_tf)):              # nothing before, nothing past what fits, nothing at all through NULL
        assert np.all(buf[:32] == FILL32) and np.all(buf[32 + (wrote if want else 0):] == FILL32)
    return int(total.value), loff[8:8 + cnt + 1].copy(), docs[32:32 + wrote].astype(np.int64), tf[32:32 + wrote].astype(np.int64)


def raw_topk(ix, pats, k, want_docs=True, want_tf=True):
    """sa_amd_index_doc_topk with canaries -> (top_off, docs, tf)"""
    data, off, cnt = sa._pattern_batch(pats)
    toff = np.full(cnt + 1 + 16, -7, dtype=np.int64)
    docs = np.full(cnt * k + 64, FILL32, dtype=np.uint32)
    tf = np.full(cnt * k + 64, FILL32, dtype=np.uint32)
    rc = sa.lib().sa_amd_index_doc_topk(ix._h, data.ctypes.data, off.ctypes.data, cnt, k, toff[8:].ctypes.data, docs[32:].ctypes.data if want_docs else None,
                                        tf[32:].ctypes.data if want_tf else None)
    assert rc == 0
    assert np.all(toff[:8] == -7) and np.all(toff[8 + cnt + 1:] == -7)
    wrote = int(toff[8 + cnt])
    assert 0 <= wrote <= cnt * k
    for buf, want in ((docs, want_docs), (tf, want_tf)):
        assert np.all(buf[:32] == FILL32) and np.all(buf[32 + (wrote if want else 0):] == FILL32)
    return toff[8:8 + cnt + 1].copy(), docs[32:32 + wrote].astype(np.int64), tf[32:32 + wrote].astype(np.int64)


def check_tf(ix, ans, pats, chunk=-1, key=None, route=None):
    """doc_tf and its statistics against the model's answers `ans` (answers_definition)"""
    prev = sa.docs_set_chunk(chunk)
    try:
        total, loff, docs, tf = raw_tf(ix, pats, sum(a[1].size for a in ans) + 5)
        st = sa.last_doc_tf_stats()
    finally:
        sa.docs_set_chunk(prev)
    df = [a[1].size for a in ans]
    assert total == sum(df) and np.array_equal(loff, np.concatenate([[0], np.cumsum(df)]))
    for q, (occ, ls, t) in enumerate(ans):
        assert np.array_equal(docs[loff[q]:loff[q + 1]], ls) and np.array_equal(tf[loff[q]:loff[q + 1]], t), (q, pats[q][:16])
        assert int(tf[loff[q]:loff[q + 1]].sum()) == occ - (0 if pats[q] else 1)
    eff = sa.DOC_CHUNK_DEFAULT if chunk < 0 else min(max(chunk, sa.DOC_CHUNK_MIN), sa.DOC_CHUNK_MAX)
    want = {"patterns": len(pats), "occ_sum": sum(a[0] for a in ans), "df_sum": total, "tf_sum": int(sum(a[2].sum() for a in ans)),
            "topk_entries": 0, "pieces": 0, "rounds": 0, "k": 0, "piece": 0, "chunk": eff}
    assert {f: st[f] for f in want} == want, (st, want)
    assert st["table_loads"] >= 2 * total                              # (every bound loads at least once: tf >= 1)
    if key is not None:
        same_for_every_route(key, route, loff, docs, tf)


def check_topk(ix, ans, pats, k, piece=-1, chunk=-1, key=None, route=None):
    """doc_topk and its statistics against the full sort of the model's answers and the model's plan of the reduction"""
    prev = sa.docs_set_chunk(chunk), sa.docs_set_topk_piece(piece)
    try:
        toff, docs, tf = raw_topk(ix, pats, k)
        st = sa.last_doc_tf_stats()
    finally:
        sa.docs_set_chunk(prev[0])
        sa.docs_set_topk_piece(prev[1])
    df = [a[1].size for a in ans]
    assert np.array_equal(toff, np.concatenate([[0], np.cumsum(np.minimum(df, k))]))
    for q, (occ, ls, t) in enumerate(ans):
        wd, wt = topk_definition(ls, t, k)
        assert np.array_equal(docs[toff[q]:toff[q + 1]], wd) and np.array_equal(tf[toff[q]:toff[q + 1]], wt), (q, pats[q][:16], k, piece)
    P = effective_piece(sa.DOC_TOPK_PIECE_DEFAULT if piece < 0 else piece, k)
    rounds, pieces, final = plan_definition(df, P, k)
    eff = sa.DOC_CHUNK_DEFAULT if chunk < 0 else min(max(chunk, sa.DOC_CHUNK_MIN), sa.DOC_CHUNK_MAX)
    want = {"patterns": len(pats), "occ_sum": sum(a[0] for a in ans), "df_sum": sum(df), "tf_sum": int(sum(a[2].sum() for a in ans)),
            "topk_entries": int(toff[-1]), "pieces": pieces, "rounds": rounds, "k": k, "piece": P, "chunk": eff}
    assert {f: st[f] for f in want} == want, (st, want)
    assert final == np.minimum(df, k).tolist()
    if key is not None:
        same_for_every_route(key, route, toff, docs, tf)
    return st


def make_index(t, arr, off, enable=True):
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents(off)
    if enable:
        ix.enable_doc_freq()
    return ix


def test_known_answers(oracle):
    t = _u8(EXAMPLE_TEXT)
    ix = make_index(t, oracle.sais(t), EXAMPLE_OFF)
    got = ix.doc_tf([b"a", b"bra", b"", b"zz"])
    assert [(d.tolist(), f.tolist()) for d, f in got] == [([3, 0, 2], [2, 2, 1]), ([3, 0], [1, 1]), ([3, 0, 2], [4, 4, 3]), ([], [])]
    assert all(d.dtype == np.uint32 and f.dtype == np.uint32 for d, f in got)
    top = {k: [(d.tolist(), f.tolist()) for d, f in ix.doc_topk([b"a", b"", b"zz"], k)] for k in (1, 2, 5, sa.DOC_TOPK_MAX)}
    assert top[1] == [([0], [2]), ([0], [4]), ([], [])]
    assert top[2] == [([0, 3], [2, 2]), ([0, 3], [4, 4]), ([], [])]
    assert top[5] == top[sa.DOC_TOPK_MAX] == [([0, 3, 2], [2, 2, 1]), ([0, 3, 2], [4, 4, 3]), ([], [])]
    assert ix.doc_tf([]) == [] and ix.doc_topk([], 3) == []
    for k in (0, sa.DOC_TOPK_MAX + 1):
        with pytest.raises(sa.SuffixArrayError):
            ix.doc_topk([b"a"], k)
    ix.close()
    s = sa.SuffixArray(t)                                              # the same three on the lazily made index
    s.set_documents(EXAMPLE_OFF)
    s.enable_doc_freq()
    assert [x.tolist() for x in s.doc_tf([b"bra"])[0]] == [[3, 0], [1, 1]] and [x.tolist() for x in s.doc_topk([b"a"], 2)[0]] == [[0, 3], [2, 2]]


def test_queries_need_the_table_and_a_new_collection_drops_it(oracle):
    t, tb = english(9000, 9)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t, arr)
    pats = some_patterns(tb, 10)
    with pytest.raises(sa.SuffixArrayError):
        ix.enable_doc_freq()                                           # no collection
    first, second = random_table(t.size, 40, 1), random_table(t.size, 2000, 2)
    for off in (first, second):
        ix.set_documents(off)
        for call in (lambda: ix.doc_tf(pats), lambda: ix.doc_topk(pats, 3)):
            with pytest.raises(sa.SuffixArrayError) as e:              # before enable_doc_freq, and again after a second set_documents
                call()
            assert e.value.code == -1
        assert len(ix.doc_list(pats)) == len(pats)                     # (what needs no table still answers)
        ix.enable_doc_freq()
        ix.enable_doc_freq()                                           # a no-op the second time
        ans = answers_definition(tb, off, arr, pats)
        check_tf(ix, ans, pats)
        check_topk(ix, ans, pats, 3)
    with pytest.raises(sa.SuffixArrayError):
        ix.set_documents([0, 5, 4, t.size])                            # a failed replacement keeps the collection and its table
    check_tf(ix, ans, pats)
    ix.close()


@pytest.mark.parametrize("ndocs", [1, 5])
def test_empty_text(oracle, ndocs):
    t = np.zeros(0, dtype=np.uint8)
    ix = make_index(t, oracle.sais(t), [0] * (ndocs + 1))
    assert [(d.size, f.size) for d, f in ix.doc_tf([b"", b"a"])] == [(0, 0), (0, 0)]
    assert [(d.size, f.size) for d, f in ix.doc_topk([b"", b"a"], 4)] == [(0, 0), (0, 0)]
    ix.close()


def test_tiny_texts(oracle):
    for b in (b"a", b"ab", b"aa", b"aba"):
        t = _u8(b)
        arr = oracle.sais(t)
        for off in ([0, len(b)], list(range(len(b) + 1)), [0, 0, 1, len(b), len(b)]):
            ix = make_index(t, arr, off)
            pats = [b"", b"a", b"b", b"ab", b"ba", b"c"]
            ans = answers_definition(b, off, arr, pats)
            check_tf(ix, ans, pats, chunk=64)
            check_topk(ix, ans, pats, 1, piece=64)
            check_topk(ix, ans, pats, 2)
            ix.close()


@pytest.mark.parametrize("ndocs", [1, 2, S - 1, S, S + 1])
def test_collections_around_the_sample_count(oracle, ndocs):
    t, tb = english(20000, 5)
    arr = oracle.sais(t)
    off = random_table(t.size, ndocs, ndocs)
    ix = make_index(t, arr, off)
    pats = some_patterns(tb, ndocs) + [b"e", b"th"]
    ans = answers_definition(tb, off, arr, pats)
    check_tf(ix, ans, pats)
    check_topk(ix, ans, pats, 10)
    ix.close()


def test_more_than_65536_documents(oracle):
    t, tb = english(300000, 6)
    arr = oracle.sais(t)
    off = random_table(t.size, 70001, 3)
    ix = make_index(t, arr, off)
    pats = some_patterns(tb, 8) + [b"e", b"th", b" "]
    ans = answers_definition(tb, off, arr, pats)
    assert max(a[1].size for a in ans) > 40000
    check_tf(ix, ans, pats)
    check_topk(ix, ans, pats, 5)
    check_topk(ix, ans, pats, 1024, piece=64)
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
    ix = make_index(t, arr, off)
    pats = some_patterns(tb, 9)
    ans = answers_definition(tb, off, arr, pats)
    assert ans[0][2].tolist() == [int(off[d + 1] - off[d]) for d in ans[0][1]]     # the empty pattern: the documents' lengths
    check_tf(ix, ans, pats)
    check_topk(ix, ans, pats, 7, piece=64)
    ix.close()


def test_galloping_edges(oracle):
    """one repeated byte in documents of 1, 2, 63, 64, 65 and 4097 bytes: the second bound lies 1, 2, 63, 64, 65 entries and whole
    documents behind the first"""
    lens = [1, 2, 63, 64, 65, 4097]
    t = np.full(sum(lens), ord("a"), dtype=np.uint8)
    tb = t.tobytes()
    arr = oracle.sais(t)
    off = np.concatenate([[0], np.cumsum(lens)])
    ix = make_index(t, arr, off)
    pats = [b"a", b"a" * 64, b"", b"a" * 4097, b"a" * 4098]
    ans = answers_definition(tb, off, arr, pats)
    assert sorted(ans[0][2].tolist()) == lens and sorted(ans[1][2].tolist()) == [1, 2, 63, 64, 65, 4097 - 63]
    for chunk in (64, -1):
        check_tf(ix, ans, pats, chunk=chunk)
    check_topk(ix, ans, pats, 3)
    ix.close()


def test_documents_that_span_several_units(oracle):
    t, tb = english(20000, 21)
    arr = oracle.sais(t)
    off = random_table(t.size, 5, 4)
    ix = make_index(t, arr, off)
    pats = [b"e", b"", b"th", b" ", b"zq"]
    ans = answers_definition(tb, off, arr, pats)
    assert max(ans[0][2]) > 16 * 64                                    # the slots of "e" of one document lie in more than sixteen units of 64
    for chunk in (64, 100, 4096):
        check_tf(ix, ans, pats, chunk=chunk, key="units", route=chunk)
    ix.close()


def test_listing_parity_capacities_and_null_outputs(oracle):
    t, tb = english(20000, 16)
    arr = oracle.sais(t)
    off = random_table(t.size, 300, 10)
    ix = make_index(t, arr, off)
    pats = [b"e", b"zq", b"th", b"", b"and"]
    ans = answers_definition(tb, off, arr, pats)
    flat_d, flat_t = np.concatenate([a[1] for a in ans]), np.concatenate([a[2] for a in ans])
    total = flat_d.size
    l_total, l_off, l_docs = raw_list(ix, pats, total)
    before = sa.last_docs_stats()
    assert l_total == total and np.array_equal(l_docs, flat_d)
    for capacity in (0, 1, total - 1, total, total + 1000):
        got_total, loff, docs, tf = raw_tf(ix, pats, capacity)
        assert got_total == total and np.array_equal(loff, l_off)      # the listing's documents, order and offsets
        assert np.array_equal(docs, flat_d[:capacity]) and np.array_equal(tf, flat_t[:capacity])
        st = sa.last_doc_tf_stats()
        assert st["df_sum"] == total and st["tf_sum"] == int(flat_t[:capacity].sum())
    for want_docs, want_tf in ((True, False), (False, True), (False, False)):
        got_total, loff, docs, tf = raw_tf(ix, pats, total, want_docs, want_tf)
        assert got_total == total and np.array_equal(loff, l_off)
        assert (not want_docs or np.array_equal(docs, flat_d)) and (not want_tf or np.array_equal(tf, flat_t))
        toff, docs, tf = raw_topk(ix, pats, 4, want_docs, want_tf)
        wd = np.concatenate([topk_definition(a[1], a[2], 4)[0] for a in ans])
        wt = np.concatenate([topk_definition(a[1], a[2], 4)[1] for a in ans])
        assert (not want_docs or np.array_equal(docs, wd)) and (not want_tf or np.array_equal(tf, wt))
    assert sa.last_docs_stats() == before                              # the new calls leave doc_list's statistics alone
    ix.close()


def _reduction_case(oracle, cache={}):
    """200 000 bytes in 5000 documents: "e" and " " occur in thousands of them"""
    if not cache:
        t, tb = english(200000, 23)
        arr = oracle.sais(t)
        off = random_table(t.size, 5000, 13)
        pats = [b"e", b"\x01nope", tb[70000:70060], b" ", b"the", b"", b"qu", tb[1000:1006]]
        cache.update(t=t, arr=arr, off=off, pats=pats, ans=answers_definition(tb, off, arr, pats))
    return cache


@pytest.mark.parametrize("piece", [64, 128, -1])
def test_reduction_pieces_and_k(oracle, piece):
    c = _reduction_case(oracle)
    ix = make_index(c["t"], c["arr"], c["off"])
    df = [a[1].size for a in c["ans"]]
    assert df[0] >= 40 * 64 and df[1] == 0 and df[2] == 1 and 2 < df[4] < 1024       # a batch of df = 0, 1, hundreds and thousands
    small = df[4]
    for k in (1, 2, small - 1, small, small + 1, 1024):
        check_topk(ix, c["ans"], c["pats"], k, piece=piece, key=("reduction", k), route=piece)
    st = check_topk(ix, c["ans"], c["pats"], 16, piece=piece, key=("reduction", 16), route=piece)
    if piece == 64:
        # the longest listing decides: "" with 4939 documents -> 78 pieces -> 1243 keys -> 20 -> 320 -> 5 -> 80 -> 2 -> 32 -> 1 piece:
        # five rounds ("e" alone, 4057 documents, would take four); check_topk has compared the figure with the model's plan
        assert st["rounds"] == 5 >= 3 and st["piece"] == 64
    ix.close()


def test_ties_are_ordered_by_document(oracle):
    """fifty identical documents: every tf is equal, the top k are the k smallest ids"""
    doc = english(400, 24)[0]
    t = np.tile(doc, 50)
    arr = oracle.sais(t)
    off = np.arange(51) * doc.size
    ix = make_index(t, arr, off)
    pats = [b"e", bytes(doc[10:14]), b" "]
    ans = answers_definition(t.tobytes(), off, arr, pats)
    assert all(a[1].size == 50 and len(set(a[2].tolist())) == 1 for a in ans)
    for k, piece in ((7, 64), (7, -1), (50, 64), (60, 128)):
        toff, docs, tf = raw_topk(ix, pats, k)
        assert docs[:toff[1]].tolist() == list(range(min(k, 50)))
        check_topk(ix, ans, pats, k, piece=piece)
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
    ix.enable_doc_freq()
    pats = some_patterns(tb, 15, 30) + [b"e", b"th", b"the ", b"zq", b"q\x00"]
    ans = answers_definition(tb, off, arr, pats)
    for chunk in (sa.DOC_CHUNK_MIN, 77, -1):
        check_tf(ix, ans, pats, chunk=chunk, key="tf_routes", route=(tables, chunk))
        for piece in (64, 128, -1):
            check_topk(ix, ans, pats, 5, piece=piece, chunk=chunk, key="topk_routes", route=(tables, chunk, piece))
    ix.close()


def test_one_mebibyte(oracle):
    t = corpus.english_corpus(1 << 20, 11)
    tb = t.tobytes()
    arr = oracle.sais(t)
    off = random_table(t.size, 4096, 7)
    ix = make_index(t, arr, off)
    pats = some_patterns(tb, 12, 20) + [b"e", b" ", b"t", b"a"]
    ans = answers_definition(tb, off, arr, pats)
    assert ans[pats.index(b" ")][0] > 10**5
    check_tf(ix, ans, pats)
    check_topk(ix, ans, pats, 10)
    check_topk(ix, ans, pats, 100, piece=256)
    ix.close()


def test_two_threads_query_one_index(oracle):
    t, tb = english(40000, 17)
    arr = oracle.sais(t)
    off = random_table(t.size, 900, 11)
    ix = make_index(t, arr, off)
    batches = [some_patterns(tb, 20 + j, 25) + [b"e", b" "] for j in range(2)]
    exp = [answers_definition(tb, off, arr, b) for b in batches]
    errors = []

    def work(j):
        try:
            sa.docs_set_topk_piece(64 if j else 128)                   # (the switches are the calling thread's)
            sa.docs_set_chunk(64 if j else 500)
            for _ in range(4):
                got = ix.doc_tf(batches[j])
                assert all(np.array_equal(d, a[1]) and np.array_equal(f, a[2]) for (d, f), a in zip(got, exp[j]))
                top = ix.doc_topk(batches[j], 9)
                st = sa.last_doc_tf_stats()
                assert (st["piece"], st["chunk"], st["k"]) == (64 if j else 128, 64 if j else 500, 9)
                for (d, f), a in zip(top, exp[j]):
                    wd, wt = topk_definition(a[1], a[2], 9)
                    assert np.array_equal(d, wd) and np.array_equal(f, wt)
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.docs_set_topk_piece(-1) == sa.DOC_TOPK_PIECE_DEFAULT    # the workers' switches were their own: this thread's is untouched
    ix.close()


def test_plain_second_bound_of_the_diagnostic_library_gives_the_same_answers(oracle):
    """the diagnostic library keeps the plain binary search for the second bound of the tf kernel beside the galloping one (the
    A/B of tools/doc_tf_bench.py): both give the model's answers, and the gallop's edges are in the batch"""
    D = sa.diag_lib()
    vp = ctypes.c_void_p
    D.sa_amd_index_create.argtypes = [vp, ctypes.c_int32, vp, vp]
    D.sa_amd_index_destroy.argtypes = [vp]
    D.sa_amd_index_destroy.restype = None
    D.sa_amd_index_set_documents.argtypes = [vp, vp, ctypes.c_int64]
    D.sa_amd_index_enable_doc_freq.argtypes = [vp]
    D.sa_amd_index_doc_tf.argtypes = [vp, vp, vp, ctypes.c_int32, vp, vp, vp, ctypes.c_int64, vp]
    D.sa_amd_debug_doc_tf_bounds.argtypes = [ctypes.c_int32]
    lens = [1, 2, 63, 64, 65, 4097]
    cases = [(np.full(sum(lens), ord("a"), dtype=np.uint8), np.concatenate([[0], np.cumsum(lens)]), [b"a", b"a" * 64, b"", b"b"])]
    t, tb = english(30000, 14)
    cases.append((t, random_table(t.size, 500, 9), some_patterns(tb, 15, 30) + [b"e", b"th", b" "]))
    for t, off, pats in cases:
        arr = oracle.sais(t)
        ans = answers_definition(t.tobytes(), off, arr, pats)
        want_d, want_t = np.concatenate([a[1] for a in ans]), np.concatenate([a[2] for a in ans])
        h = vp()
        offs = np.asarray(off, dtype=np.uint32)
        assert D.sa_amd_index_create(t.ctypes.data, t.size, arr.ctypes.data, ctypes.byref(h)) == 0
        try:
            assert D.sa_amd_index_set_documents(h, offs.ctypes.data, offs.size - 1) == 0 and D.sa_amd_index_enable_doc_freq(h) == 0
            data, poff, cnt = sa._pattern_batch(pats)
            for mode in (1, 0):
                prev = D.sa_amd_debug_doc_tf_bounds(mode)
                try:
                    loff = np.zeros(cnt + 1, dtype=np.int64)
                    docs, tf = np.zeros(want_d.size + 1, dtype=np.uint32), np.zeros(want_d.size + 1, dtype=np.uint32)
                    total = ctypes.c_int64(-1)
                    assert D.sa_amd_index_doc_tf(h, data.ctypes.data, poff.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, tf.ctypes.data,
                                                 docs.size, ctypes.byref(total)) == 0
                finally:
                    D.sa_amd_debug_doc_tf_bounds(prev)
                assert total.value == want_d.size and np.array_equal(docs[:-1], want_d) and np.array_equal(tf[:-1], want_t), mode
        finally:
            D.sa_amd_index_destroy(h)
