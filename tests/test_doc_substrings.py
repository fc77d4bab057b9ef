"""GPU suite for the document frequency of the repeated substrings: sa_amd_index_doc_substrings bit for bit
against the model of test_doc_substrings_abi.py over the oracle's suffix array and oracle_lcp_kasai, at the sizes where the
kernels change shape (one block of the fan-out of 32, the tile of 1024, three and four levels of minima), over collections
from one document to every byte its own, with canaries around the three outputs, cut capacities, NULL outputs, the statistics,
and agreement with repeated_substrings and doc_search."""
import ctypes
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_substrings import _families, reference
from test_substrings_abi import ALL, BY_COUNT, BY_COVER, BY_LENGTH
from test_doc_substrings_abi import BY_DOCS, doc_table, prev_slots, rmq_bound, run_doc_query, slot_docs, walk_counters

pytestmark = pytest.mark.gpu

CANARY = 0xA7A7A7A7
OLD_ORDERS = (BY_COUNT, BY_LENGTH, BY_COVER)


def collections(n, seed=0):
    """name -> doc_off of the issue's list for a text of n bytes"""
    rng = np.random.default_rng(7000 + n + seed)
    ndocs = min(1000, max(n // 3, 1))
    cuts = np.sort(rng.integers(0, n + 1, max(ndocs - 7, 0)))
    mid = int(cuts[cuts.size // 2]) if cuts.size else n // 2
    many = np.sort(np.concatenate(([0, 0, 0], cuts, [mid, mid], [n, n, n])))          # empty documents in front, in the middle, at the end
    return {"one": np.array([0, n]), "bytes": np.arange(n + 1) if n else np.array([0, 0]), "halves": np.array([0, n // 2, n]), "many": many,
            "at32": np.array([0, min(32, n), n]), "at1024": np.array([0, min(1024, n), n])}


def doc_ref(ref, cname, off):
    """the node table with df of (text, collection), computed once and kept in the text's cache"""
    t, arr, lcp, _, cache = ref
    key = ("doc", cname)
    if key not in cache:
        tab = doc_table(lcp, arr, off)
        if t.size <= 2100 or (t.size <= 33000 and cname == "at1024"):  # the kernels' walk, word for word, where Python can afford it
            tab.update(walk_counters(lcp, prev_slots(slot_docs(arr, off)))[0])
        cache[key] = (tab, {})
    return cache[key]


def model(ref, cname, off, flt=(1, 0, 2), min_docs=1, order=ALL, k=0):
    """rows, df, pos and counters of one query; the full ranking of (filter, min_docs, order) is computed once and cut at k"""
    tab, ranked = doc_ref(ref, cname, off)
    key = (flt, min_docs, order)
    if key not in ranked:
        rows, df, _, st = run_doc_query(tab, *flt, min_docs=min_docs, order=order, k=1 << 62)
        ranked[key] = (rows, df, ref[1][rows[:, 0]].astype(np.uint32), st)
    rows, df, pos, st = ranked[key]
    return (rows, df, pos, st) if order == ALL else (rows[:k], df[:k], pos[:k], st)


def check_stats(ref, cname, off, flt, min_docs, order, k, got=None):
    got = sa.last_doc_substr_stats() if got is None else got
    tab, _ = doc_ref(ref, cname, off)
    st = model(ref, cname, off, flt, min_docs, order, k)[3]
    for key, val in st.items():
        assert got[key] == val, (key, got, st)
    n = ref[0].size
    assert got["rmq_max"] <= rmq_bound(n) and got["rmq_far"] <= got["pairs"] <= got["rmq_steps"]
    for key in ("rmq_steps", "rmq_max"):
        if key in tab:
            assert got[key] == tab[key], (key, got[key], tab[key])
    assert got["sorted"] == (0 if order == ALL else min(k, st["selected"])) and got["select_passes"] <= 8 and got["readbacks"] >= 1
    if order == ALL or k >= st["selected"]:
        assert got["select_passes"] == 0
    return got


def check_one(ix, ref, cname, off, flt, min_docs, order, k, name):
    rows, df, pos, _ = model(ref, cname, off, flt, min_docs, order, k)
    got, gdf, gpos = ix.doc_substrings(*flt, min_docs=min_docs, order=order, k=k, positions=True)
    what = (name, cname, flt, min_docs, order, k)
    assert got.dtype == np.uint32 and got.shape == rows.shape and np.array_equal(got, rows), what
    assert gdf.dtype == np.uint32 and np.array_equal(gdf, df), what
    assert gpos.dtype == np.uint32 and np.array_equal(gpos, pos), what
    check_stats(ref, cname, off, flt, min_docs, order, k)


def check_collection(ix, ref, cname, off, name, other_order=BY_COUNT, flt=(1, 0, 2)):
    """the issue's queries over one (text, collection): every min_docs unranked; BY_DOCS and one old order over every k"""
    ix.set_documents(off)
    ndocs = len(off) - 1
    for md in sorted({1, 2, 3, ndocs, ndocs + 1}):
        check_one(ix, ref, cname, off, flt, md, ALL, 0, name)
    for order, md in ((BY_DOCS, 1), (BY_DOCS, 2), (other_order, 2)):
        sel = model(ref, cname, off, flt, md)[3]["selected"]
        for k in sorted({1, 2, max(sel - 1, 1), max(sel, 1), sel + 1, 100000}):
            check_one(ix, ref, cname, off, flt, md, order, k, name)


def check_text(oracle, name, b, which=None, flt=(1, 0, 2)):
    ref = reference(oracle, name, lambda: b)
    t, arr = ref[0], ref[1]
    ix = sa.DeviceIndex(t, arr)
    for j, (cname, off) in enumerate(collections(t.size).items()):
        if which is None or cname in which:
            check_collection(ix, ref, cname, off, name, OLD_ORDERS[j % 3], flt)          # set_documents again: the answers follow
    ix.close()
    return ref


def raw(ix, q, capacity, want_df=True, want_pos=True):
    """the C entry on numpy buffers with 64 canary words on either side of rows, df and pos -> (total, rows, df, pos)"""
    rows = np.full(4 * capacity + 128, CANARY, dtype=np.uint32)
    df = np.full(capacity + 128, CANARY, dtype=np.uint32)
    pos = np.full(capacity + 128, CANARY, dtype=np.uint32)
    total = ctypes.c_int64(-1)
    rc = sa.lib().sa_amd_index_doc_substrings(ix._h, ctypes.byref(q), rows[64:].ctypes.data if capacity else None,
                                              df[64:].ctypes.data if want_df else None, pos[64:].ctypes.data if want_pos else None,
                                              capacity, ctypes.byref(total))
    assert rc == 0
    wrote = min(int(total.value), capacity)
    assert np.all(rows[:64] == CANARY) and np.all(rows[64 + 4 * wrote:] == CANARY)
    assert np.all(df[:64] == CANARY) and np.all(df[64 + (wrote if want_df else 0):] == CANARY)
    assert np.all(pos[:64] == CANARY) and np.all(pos[64 + (wrote if want_pos else 0):] == CANARY)
    return int(total.value), rows[64:64 + 4 * wrote].reshape(-1, 4), df[64:64 + wrote], pos[64:64 + wrote]


def test_header_examples():
    ix = sa.DeviceIndex(b"abracadabra")
    with pytest.raises(ValueError):
        ix.doc_substrings()                                             # no collection set
    ix.set_documents([0, 4, 4, 7, 11])
    rows, df, pos = ix.doc_substrings(positions=True)
    subs = {bytes(b"abracadabra"[p:p + d]): (int(c), int(f)) for (lo, c, d, par), f, p in zip(rows.tolist(), df.tolist(), pos.tolist())}
    assert subs == {b"a": (5, 3), b"abra": (2, 2), b"bra": (2, 2), b"ra": (2, 2)}
    st = sa.last_doc_substr_stats()
    assert (st["nodes"], st["selected"], st["df_sum"], st["max_df"], st["pairs"]) == (4, 4, 9, 3, 8)
    rows, df = ix.doc_substrings(order=sa.SUBSTR_BY_DOCS, k=1)
    assert rows.tolist() == [[1, 5, 1, 0]] and df.tolist() == [3]
    rows, df = ix.doc_substrings(min_docs=2, order=sa.SUBSTR_BY_LENGTH, k=1)
    assert rows.tolist() == [[2, 2, 4, 1]] and df.tolist() == [2]       # the longest substring common to two documents: "abra"
    assert ix.doc_substrings(min_docs=4)[0].shape == (0, 4)
    ix.set_documents([0, 11])
    assert ix.doc_substrings()[1].tolist() == [1, 1, 1, 1]
    ix.close()
    s = sa.SuffixArray(b"aaaa")
    s.set_documents([0, 2, 4])
    rows, df = s.doc_substrings()
    assert rows[:, 1:3].tolist() == [[4, 1], [3, 2], [2, 3]] and df.tolist() == [2, 2, 1]


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_texts(oracle, n):
    for name, b in _families(n).items():
        check_text(oracle, f"{name}_{n}", b)


@pytest.mark.parametrize("n", [31, 32, 33, 1023, 1024, 1025])
def test_sizes_where_a_stage_changes(oracle, n):
    """one block of the fan-out, the tile edge: the walk's loads are compared word for word with its replica"""
    for name, b in _families(n).items():
        check_text(oracle, f"{name}_{n}", b)


@pytest.mark.parametrize("n", [32767, 32769])
def test_third_level_of_minima(oracle, n):
    for j, (name, b) in enumerate(_families(n).items()):
        check_text(oracle, f"{name}_{n}", b, which=("one", "bytes", "many") if j % 2 else ("halves", "many", "at32", "at1024"))


def test_dna_70000(oracle):
    check_text(oracle, "dna_70000", corpus.dna(70000, 11), which=("many", "halves"), flt=(9, 0, 2))


def test_english_256k(oracle):
    check_text(oracle, "english_256k", corpus.english_corpus(256 << 10, 5), which=("many", "at1024"), flt=(2, 3, 2))


def test_text_twice_with_the_boundary_in_the_middle(oracle):
    h = corpus.english_corpus(20000, 9).tobytes()
    ref = check_text(oracle, "english_twice", h + h, which=("halves",))
    tab, _ = doc_ref(ref, "halves", None)
    ext = np.append(ref[1].astype(np.int64), 1 << 40)
    first = np.minimum.reduceat(ext, np.stack([tab["lo"], tab["lo"] + tab["count"]], axis=1).ravel())[::2]      # the node's leftmost occurrence
    inside = first + tab["depth"] <= len(h)                                 # it lies inside the first half: its copy is in the second
    assert inside.sum() > 1000 and (tab["df"][inside] == 2).all()


def test_four_levels_and_pairs_that_span_half_the_array(oracle):
    """1 048 576 + 4 097 bytes over two letters.  Documents of two bytes: the suffixes of "ab" stand in the two halves of the
    array, so most pairs are half the array long and climb to the top level; about 1000 documents beside it"""
    n = (1 << 20) + 4097
    ref = reference(oracle, "random2_4levels", lambda: np.random.default_rng(41).integers(97, 99, n, dtype=np.uint8))
    t, arr = ref[0], ref[1]
    ix = sa.DeviceIndex(t, arr)
    two = np.concatenate((np.arange(0, n, 2), [n]))
    for cname, off in (("two_bytes", two), ("many", collections(n)["many"])):
        ix.set_documents(off)
        ndocs = len(off) - 1
        check_one(ix, ref, cname, off, (1, 0, 2), 2, ALL, 0, "4levels")
        st = sa.last_doc_substr_stats()
        assert rmq_bound(n) == 93 * 4 + 32 and 0 < st["rmq_max"] <= rmq_bound(n) and st["rmq_far"] > 0.9 * st["pairs"]
        check_one(ix, ref, cname, off, (1, 0, 2), 1, BY_DOCS, 1000, "4levels")
        check_one(ix, ref, cname, off, (1, 0, 2), ndocs // 2, BY_LENGTH, 1, "4levels")
        check_one(ix, ref, cname, off, (2, 3, 2), 3, BY_COVER, 7, "4levels")
    P = prev_slots(slot_docs(arr, two))
    far = np.nonzero(P >= 0)[0]
    # half of the documents are "ab" or "ba"; their two slots are uniform in either half, so 7 / 8 of them lie more than n / 4 apart
    assert ((far - P[far]) > n // 4).mean() > 0.4
    ix.close()


def test_buffers_capacities_and_null_outputs(oracle):
    ref = reference(oracle, "fibonacci_1025", lambda: _families(1025)["fibonacci"])
    off = collections(1025)["many"]
    ix = sa.DeviceIndex(ref[0], ref[1])
    ix.set_documents(off)
    for order, k, md in ((ALL, 0, 2), (BY_DOCS, 7, 1), (BY_COVER, 100000, 3)):
        rows, df, pos, _ = model(ref, "many", off, (1, 0, 2), md, order, k)
        total = rows.shape[0]
        assert total > 5
        q = sa.DocSubstrQuery(1, 0, 2, order, k, md)
        for cap in sorted({0, total - 1, total, total + 5}):
            t2, grows, gdf, gpos = raw(ix, q, cap)
            assert t2 == total and np.array_equal(grows, rows[:cap]) and np.array_equal(gdf, df[:cap]) and np.array_equal(gpos, pos[:cap])
            check_stats(ref, "many", off, (1, 0, 2), md, order, k)
        t2, grows, _, gpos = raw(ix, q, total + 5, want_df=False)
        assert t2 == total and np.array_equal(grows, rows) and np.array_equal(gpos, pos)
        t2, grows, gdf, _ = raw(ix, q, total + 5, want_pos=False)
        assert t2 == total and np.array_equal(grows, rows) and np.array_equal(gdf, df)
        t2, grows, _, _ = raw(ix, q, total, want_df=False, want_pos=False)
        assert t2 == total and np.array_equal(grows, rows)
    ix.close()


def test_agreement_with_repeated_substrings_and_doc_search(oracle):
    """min_docs = 1 and the old orders: the rows and pos of repeated_substrings, bit for bit; df of sampled rows: doc_search's.
    The same with the LCP table and the frequency table enabled"""
    ref = reference(oracle, "dna_70000", lambda: corpus.dna(70000, 11))
    t = ref[0]
    ix = sa.DeviceIndex(t, ref[1])
    ix.set_documents(collections(t.size)["many"])
    rng = np.random.default_rng(3)
    for tables in (False, True):
        if tables:
            ix.enable_lcp()
            ix.enable_doc_freq()
        for flt, order, k in (((1, 0, 2), ALL, 0), ((9, 0, 2), BY_COUNT, 500), ((2, 3, 2), BY_COVER, 77), ((1, 0, 3), BY_LENGTH, 100000)):
            rows, pos = ix.repeated_substrings(*flt, order=order, k=k, positions=True)
            got, gdf, gpos = ix.doc_substrings(*flt, min_docs=1, order=order, k=k, positions=True)
            assert np.array_equal(got, rows) and np.array_equal(gpos, pos), (tables, flt, order)
            pick = rng.permutation(rows.shape[0])[:60]
            occ, df = ix.doc_search([t[int(pos[r]):int(pos[r]) + int(rows[r, 2])].tobytes() for r in pick])
            assert np.array_equal(occ, rows[pick, 1]) and np.array_equal(df, gdf[pick]), (tables, flt, order)
    ix.close()


def test_errors_with_an_index():
    L = sa.lib()
    ix = sa.DeviceIndex(b"mississippi")
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)

    def call(q, rows=p, cap=4, total=c):
        return L.sa_amd_index_doc_substrings(ix._h, None if q is None else ctypes.byref(q), rows, p, p, cap, total)
    ok = sa.DocSubstrQuery(1, 0, 2, ALL, 0, 1)
    assert call(ok) == -1                                               # no collection set
    ix.set_documents([0, 5, 11])
    Q = sa.DocSubstrQuery
    for bad in (Q(0, 0, 2, ALL, 0, 1), Q(5, 4, 2, ALL, 0, 1), Q(1, -1, 2, ALL, 0, 1), Q(1, 0, 1, ALL, 0, 1), Q(1, 0, 2, 5, 1, 1), Q(1, 0, 2, -1, 1, 1),
                Q(1, 0, 2, BY_DOCS, 0, 1), Q(1, 0, 2, BY_COUNT, -1, 1), Q(1, 0, 2, ALL, 0, 0), Q(1, 0, 2, BY_DOCS, 3, -2)):
        assert call(bad) == -1, tuple(getattr(bad, f) for f, _ in bad._fields_)
    assert call(None) == -1 and call(ok, cap=-1) == -1 and call(ok, total=None) == -1 and call(ok, rows=None) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777)                # nothing written
    assert call(ok, rows=None, cap=0) == 0 and tot.value == 6           # i, issi, p, s, si, ssi
    with pytest.raises(ValueError):
        ix.doc_substrings(min_docs=0)
    with pytest.raises(ValueError):
        ix.doc_substrings(order=sa.SUBSTR_BY_DOCS)                      # k = 0
    ix.close()


def test_statistics_of_other_features_stay(oracle):
    """the LCP build inside fills last_lcp_stats as sa_amd_lcp does; the statistics of repeated_substrings, doc_search and lz77 stay"""
    t = corpus.english_corpus(5000, 3)
    arr = oracle.sais(t)
    sa.lz77(corpus.dna(3000, 4))
    ix = sa.DeviceIndex(t, arr)
    ix.set_documents([0, 1000, 1000, 4000, 5000])
    ix.repeated_substrings(order=BY_COUNT, k=10)
    ix.doc_search([b"the", b"of"])
    before = (sa.last_lz_stats(), sa.last_substr_stats(), sa.last_docs_stats(), sa.last_doc_tf_stats(), sa.last_repeat_stats())
    assert before[0]["phrases"] > 0 and before[1]["nodes"] > 0 and before[2]["patterns"] == 2
    sa.lcp(t, arr)
    plain = sa.last_lcp_stats()
    ix.doc_substrings(min_docs=2, order=sa.SUBSTR_BY_DOCS, k=10)
    assert (sa.last_lz_stats(), sa.last_substr_stats(), sa.last_docs_stats(), sa.last_doc_tf_stats(), sa.last_repeat_stats()) == before
    inside = sa.last_lcp_stats()
    for key in ("irreducible", "compared_bytes", "long_pairs", "readbacks"):
        assert inside[key] == plain[key], key
    ix.close()


def test_two_threads_query_one_index(oracle):
    ref = reference(oracle, "thread_english", lambda: corpus.english_corpus(60000, 21))
    off = collections(60000)["many"]
    ix = sa.DeviceIndex(ref[0], ref[1])
    ix.set_documents(off)
    queries = [((2, 3, 2), 2, BY_DOCS, 50), ((1, 0, 2), 3, ALL, 0)]
    exp = [model(ref, "many", off, *q) for q in queries]
    errors = []

    def work(j):
        try:
            flt, md, order, k = queries[j]
            for _ in range(3):
                got, gdf = ix.doc_substrings(*flt, min_docs=md, order=order, k=k)
                st = sa.last_doc_substr_stats()
                assert np.array_equal(got, exp[j][0]) and np.array_equal(gdf, exp[j][1])
                check_stats(ref, "many", off, flt, md, order, k, st)
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    ix.close()
    assert not errors, errors
