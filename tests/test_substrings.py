"""GPU suite for repeated-substring enumeration: every route, bit for bit against the model of
test_substrings_abi.py over the oracle's suffix array and oracle_lcp_kasai, at the sizes where the kernels change shape (the
fan-out of 32, the tile of 1024, three and four levels of minima), with the rows' and positions' canaries, cut capacities, NULL
outputs and the statistics."""
import ctypes
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word, thue_morse
from test_lcp import _Dev
from test_lcp_abi import _kasai
from test_substrings_abi import ALL, BY_COUNT, BY_COVER, BY_LENGTH, _golden, _u8, node_table, run_query

pytestmark = pytest.mark.gpu

CANARY = 0xA7
FILTERS = [(1, 0, 2), (2, 3, 2), (4, 4, 2), (1, 1, 3), (50, 0, 2)]
RANKED = (BY_COUNT, BY_LENGTH, BY_COVER)
STEP_BOUND = 347                                                      # 31 (K - 1) + 32 K loads a side, K <= 6
_REF = {}


def reference(oracle, name, make):
    """(text, array, LCP, node table, cache of full rankings) of a named text: computed once, shared and left unchanged"""
    if name not in _REF:
        t = _u8(make())
        arr = oracle.sais(t)
        lcp = _kasai(oracle, t, arr)
        for a in (t, arr, lcp):
            a.flags.writeable = False
        _REF[name] = (t, arr, lcp, node_table(lcp), {})
    return _REF[name]


def model(ref, flt, order=ALL, k=0):
    """rows, pos and counters of one query; the full ranking of a (filter, order) is computed once and cut at k"""
    t, arr, lcp, tab, cache = ref
    if (flt, order) not in cache:
        rows, _, st = run_query(tab, *flt, order=order, k=1 << 62)
        cache[flt, order] = (rows, arr[rows[:, 0]].astype(np.uint32), st)
    rows, pos, st = cache[flt, order]
    return (rows, pos, st) if order == ALL else (rows[:k], pos[:k], st)


def check_stats(ref, flt, order, k, got=None):
    got = sa.last_substr_stats() if got is None else got
    rows, _, st = model(ref, flt, order, k)
    for key, val in st.items():
        assert got[key] == val, (key, got, st)
    assert got["unresolved"] == ref[3]["unresolved"] or ref[0].size == 0
    assert got["far_max"] <= STEP_BOUND and got["select_passes"] <= 8 and got["readbacks"] >= 1
    assert got["sorted"] == (0 if order == ALL else min(k, st["selected"]))
    if order == ALL or k >= st["selected"]:
        assert got["select_passes"] == 0
    return got


def check_queries(ref, name, filters=FILTERS, ranked_filters=((1, 0, 2), (2, 3, 2)), use_sa=True):
    """the host form over every query of the issue's list"""
    t, arr = ref[0], ref[1]
    a = arr if use_sa else None
    for flt in filters:
        rows, pos, st = model(ref, flt)
        got, gpos = sa.repeated_substrings(t, *flt, sa=a, positions=True)
        assert got.dtype == np.uint32 and got.shape == rows.shape and np.array_equal(got, rows), (name, flt)
        assert gpos.dtype == np.uint32 and np.array_equal(gpos, pos), (name, flt)
        check_stats(ref, flt, ALL, 0)
    for flt in ranked_filters:
        sel = model(ref, flt)[2]["selected"]
        for order in RANKED:
            for k in sorted({1, 2, max(sel - 1, 1), max(sel, 1), sel + 1, 1000, 100000}):
                rows, pos, _ = model(ref, flt, order, k)
                got, gpos = sa.repeated_substrings(t, *flt, order=order, k=k, sa=a, positions=True)
                assert got.shape == rows.shape and np.array_equal(got, rows), (name, flt, order, k)
                assert np.array_equal(gpos, pos), (name, flt, order, k)
                check_stats(ref, flt, order, k)


def on_device(ref, flt, order, k, capacity, want_pos=True):
    """sa_amd_substrings_device on device buffers with a work block of exactly work_bytes, 256 canary bytes on either side of
    rows and pos; checks the canaries and that nothing is written behind the rows that exist; -> (total, rows, pos)"""
    t, arr = ref[0], ref[1]
    n = t.size
    wb = sa.substrings_work_bytes(n)
    with _Dev(n + 16, 4 * (n + 1), 16 * capacity + 512, 4 * capacity + 512, wb) as d:
        dT, dS, dR, dP, dW = d.p
        assert dW % 256 == 0
        assert d.hip.hipMemset(dR, CANARY, 16 * capacity + 512) == 0 and d.hip.hipMemset(dP, CANARY, 4 * capacity + 512) == 0
        if n:
            assert d.hip.hipMemcpy(dT, t.ctypes.data, n, 1) == 0
        assert d.hip.hipMemcpy(dS, arr.ctypes.data, 4 * (n + 1), 1) == 0
        q = sa.SubstrQuery(flt[0], flt[1], flt[2], order, k)
        total = sa.substrings_device_ptr(dT, dS, n, q, dR + 256 if capacity else 0, dP + 256 if want_pos else 0, capacity, dW, wb)
        raw, rawp = np.zeros(16 * capacity + 512, dtype=np.uint8), np.zeros(4 * capacity + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dR, raw.size, 2) == 0 and d.hip.hipMemcpy(rawp.ctypes.data, dP, rawp.size, 2) == 0
    wrote = min(total, capacity)
    assert np.all(raw[:256] == CANARY) and np.all(raw[256 + 16 * wrote:] == CANARY)
    assert np.all(rawp[:256] == CANARY) and np.all(rawp[256 + (4 * wrote if want_pos else 0):] == CANARY)
    rows = raw[256:256 + 16 * wrote].view(np.uint32).reshape(-1, 4)
    return total, rows, (rawp[256:256 + 4 * wrote].view(np.uint32) if want_pos else None)


def check_device_form(ref, name, flt=(1, 0, 2)):
    for order, k in ((ALL, 0), (BY_COVER, 7), (BY_COUNT, 100000)):
        rows, pos, st = model(ref, flt, order, k)
        total = rows.shape[0]
        for cap in sorted({0, max(total - 1, 0), total, total + 5}):
            got_total, got, gpos = on_device(ref, flt, order, k, cap)
            assert got_total == total and np.array_equal(got, rows[:cap]) and np.array_equal(gpos, pos[:cap]), (name, order, cap)
            check_stats(ref, flt, order, k)
        got_total, got, _ = on_device(ref, flt, order, k, total + 5, want_pos=False)      # pos passed as NULL
        assert got_total == total and np.array_equal(got, rows), (name, order)


def check_all_routes(ref, name):
    """the host form with the caller's array and with SA=None, the device form, the index with and without enable_lcp, the
    SuffixArray method: the same bytes"""
    t, arr = ref[0], ref[1]
    check_queries(ref, name)
    check_queries(ref, name, filters=[(1, 0, 2), (2, 3, 2)], ranked_filters=((1, 0, 2),), use_sa=False)
    check_device_form(ref, name)
    ix = sa.DeviceIndex(t, arr)
    s = sa.SuffixArray.unchecked_from_parts(t, arr)
    for with_lcp in (False, True):
        if with_lcp:
            ix.enable_lcp()
        for flt, order, k in (((1, 0, 2), ALL, 0), ((2, 3, 2), BY_COVER, 5), ((1, 0, 2), BY_COUNT, 3), ((1, 1, 3), BY_LENGTH, 100000)):
            rows, pos, _ = model(ref, flt, order, k)
            got, gpos = ix.repeated_substrings(*flt, order=order, k=k, positions=True)
            assert np.array_equal(got, rows) and np.array_equal(gpos, pos), (name, with_lcp, flt, order)
            check_stats(ref, flt, order, k)
            got = s.repeated_substrings(*flt, order=order, k=k)
            assert got.dtype == np.uint32 and np.array_equal(got, rows), (name, flt, order)
    ix.close()


def _families(n):
    rng = np.random.default_rng(1000 + n)
    h = rng.integers(97, 100, n // 2, dtype=np.uint8).tobytes()
    return {"a_run": b"a" * n, "ab_period": (b"ab" * (n // 2 + 1))[:n], "fibonacci": fibonacci_word(24)[:n],
            "thue_morse": bytes(b + 97 for b in thue_morse(n)), "twice": (h + h + b"a")[:n],
            "random2": rng.integers(97, 99, n, dtype=np.uint8).tobytes()}


def test_header_example():
    rows, pos = sa.repeated_substrings(b"banana", positions=True)
    assert rows.tolist() == [[1, 3, 1, 0], [2, 2, 3, 1], [5, 2, 2, 0]] and pos.tolist() == [5, 3, 4]
    st = sa.last_substr_stats()
    assert (st["nodes"], st["selected"], st["distinct_all"], st["distinct_selected"]) == (3, 3, 5, 5)
    assert sa.repeated_substrings(b"banana", order=sa.SUBSTR_BY_COVER, k=2).tolist() == [[2, 2, 3, 1], [5, 2, 2, 0]]
    assert sa.repeated_substrings(b"banana", max_len=1, order=sa.SUBSTR_BY_COVER, k=5).tolist() == [[1, 3, 1, 0], [5, 2, 2, 0]]
    assert sa.repeated_substrings(b"banana", min_count=3).tolist() == [[1, 3, 1, 0]]
    assert sa.repeated_substrings(bytes(range(256))).shape == (0, 4)


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_texts_all_routes(oracle, n):
    for name, b in _families(n).items():
        check_all_routes(reference(oracle, f"{name}_{n}", lambda b=b: b), f"{name}_{n}")


@pytest.mark.parametrize("n", [31, 32, 33, 1023, 1024, 1025, 2049, 32767, 32769])
def test_sizes_where_a_stage_changes(oracle, n):
    """one group of the fan-out, the tile edge, the third level of minima"""
    for name, b in _families(n).items():
        ref = reference(oracle, f"{name}_{n}", lambda b=b: b)
        if n in (33, 1025, 32769) and name in ("fibonacci", "random2"):
            check_all_routes(ref, f"{name}_{n}")
        else:
            check_queries(ref, f"{name}_{n}", ranked_filters=((1, 0, 2),))


def test_adversarial_cases(oracle):
    for name, b in adversarial_cases().items():
        check_queries(reference(oracle, "adv_" + name, lambda b=b: b), name, ranked_filters=((1, 0, 2),))


def test_golden_all_bytes_twice(oracle):
    t, _ = _golden("all_bytes_twice")
    ref = reference(oracle, "all_bytes_twice", lambda: t)
    check_all_routes(ref, "all_bytes_twice")
    assert model(ref, (1, 0, 2))[2]["nodes"] == 256


def test_dna_many_equal_values_across_tiles(oracle):
    """seeded DNA of 70 000 bytes: three levels, equal LCP values in every tile.  BY_COUNT with min_len = 9: almost every count
    is 2, so the cut key holds nearly all candidates and the result is the first k by slot"""
    ref = reference(oracle, "dna_70000", lambda: corpus.dna(70000, 11))
    check_queries(ref, "dna_70000")
    check_device_form(ref, "dna_70000", (9, 0, 2))
    flt = (9, 0, 2)
    full, _, st = model(ref, flt, BY_COUNT, 1 << 40)
    sel = st["selected"]
    twos = int((full[:, 1] == 2).sum())
    assert sel > 1000 and twos > 0.9 * sel
    for k in (1, 2, sel - twos + 1, sel // 2, sel - 1, sel, sel + 1):
        rows, pos, _ = model(ref, flt, BY_COUNT, k)
        got, gpos = sa.repeated_substrings(ref[0], *flt, order=BY_COUNT, k=k, sa=ref[1], positions=True)
        assert np.array_equal(got, rows) and np.array_equal(gpos, pos), k
        assert check_stats(ref, flt, BY_COUNT, k)["sorted"] == min(k, sel)


def test_english_256k(oracle):
    ref = reference(oracle, "english_256k", lambda: corpus.english_corpus(256 << 10, 5))
    check_queries(ref, "english_256k")
    check_device_form(ref, "english_256k", (4, 4, 2))


def test_text_twice(oracle):
    h = corpus.english_corpus(20000, 9).tobytes()
    ref = reference(oracle, "english_twice", lambda: h + h)
    check_queries(ref, "english_twice")
    assert model(ref, (50, 0, 2))[2]["selected"] > 0


def test_four_levels_equal_values_far_apart(oracle):
    """1 048 576 + 4 097 bytes over two letters: level 4 appears, and the depth-1 nodes span half the array each, so the equal
    values that the "<=" side must stop at lie hundreds of thousands of slots apart"""
    n = (1 << 20) + 4097
    ref = reference(oracle, "random2_4levels", lambda: np.random.default_rng(41).integers(97, 99, n, dtype=np.uint8))
    tab = ref[3]
    assert int(tab["count"][tab["depth"] == 1].min()) > n // 3
    check_queries(ref, "random2_4levels", ranked_filters=((1, 0, 2),))                    # all five ALL filters
    st = sa.last_substr_stats()
    assert st["unresolved"] > 0 and 0 < st["far_max"] <= STEP_BOUND
    total, rows, pos = on_device(ref, (1, 0, 2), BY_COVER, 1000, 1000)
    exp = model(ref, (1, 0, 2), BY_COVER, 1000)
    assert total == 1000 and np.array_equal(rows, exp[0]) and np.array_equal(pos, exp[1])


def test_errors(oracle):
    L = sa.lib()
    ref = reference(oracle, "adv_mississippi", lambda: b"mississippi")
    t, arr = ref[0], np.array(ref[1])
    n = t.size
    out = np.full(4 * n + 4, 0x77777777, dtype=np.uint32)
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    q = ctypes.byref(sa.SubstrQuery(1, 0, 2, ALL, 0))
    bad = arr.copy()
    bad[5] = n + 1
    assert L.sa_amd_substrings(t.ctypes.data, n, bad.ctypes.data, q, out.ctypes.data, None, n, c) == -6
    with pytest.raises(IndexError):
        sa.repeated_substrings(t, sa=bad)
    bad = arr.copy()
    bad[0], bad[3] = bad[3], bad[0]
    assert L.sa_amd_substrings(t.ctypes.data, n, bad.ctypes.data, q, out.ctypes.data, None, n, c) == -1
    with pytest.raises(ValueError):
        sa.repeated_substrings(t, sa=bad)
    assert tot.value == -5 and np.all(out == 0x77777777)                                      # nothing written
    assert L.sa_amd_substrings(None, 0, np.array([1], dtype=np.uint32).ctypes.data, q, None, None, 0, c) == -6
    assert L.sa_amd_substrings(None, 0, np.array([0], dtype=np.uint32).ctypes.data, q, None, None, 0, c) == 0 and tot.value == 0
    wb = sa.substrings_work_bytes(n)
    with _Dev(n, 4 * (n + 1), 16 * n + 512, wb + 256) as d:
        dT, dS, dO, dW = d.p
        assert d.hip.hipMemset(dO, CANARY, 16 * n + 512) == 0
        assert d.hip.hipMemcpy(dS, arr.ctypes.data, 4 * (n + 1), 1) == 0
        assert d.hip.hipMemcpy(dT, t.ctypes.data, n, 1) == 0
        tot.value = -5
        args = (dT, dS, n, q, dO + 256, None, n, c)
        assert L.sa_amd_substrings_device(*args, dW, wb - 256, None) == -1                    # 256 bytes short
        assert L.sa_amd_substrings_device(*args, dW + 4, wb, None) == -1                      # misaligned
        assert L.sa_amd_substrings_device(*args, dW + 128, wb, None) == -1
        raw = np.zeros(16 * n + 512, dtype=np.uint8)
        assert d.hip.hipMemcpy(raw.ctypes.data, dO, raw.size, 2) == 0
        assert np.all(raw == CANARY) and tot.value == -5
        assert L.sa_amd_substrings_device(*args, dW, wb, None) == 0 and tot.value == model(ref, (1, 0, 2))[0].shape[0]


def test_statistics_of_other_features_stay(oracle):
    """the LCP build inside fills last_lcp_stats as sa_amd_lcp does; last_lz_stats is not touched"""
    t = corpus.english_corpus(5000, 3)
    other = corpus.dna(3000, 4)
    sa.lz77(other)
    lz = sa.last_lz_stats()
    assert lz["phrases"] > 0
    arr = oracle.sais(t)
    sa.lcp(t, arr)
    plain = sa.last_lcp_stats()
    sa.repeated_substrings(t, order=BY_COUNT, k=10, sa=arr)
    assert sa.last_lz_stats() == lz
    inside = sa.last_lcp_stats()
    for key in ("irreducible", "compared_bytes", "long_pairs", "readbacks"):
        assert inside[key] == plain[key], key


def test_two_threads_see_their_own_statistics(oracle):
    refs = [reference(oracle, "thread_english", lambda: corpus.english_corpus(60000, 21)),
            reference(oracle, "thread_dna", lambda: corpus.dna(50000, 22))]
    queries = [((2, 3, 2), BY_COVER, 50), ((1, 0, 2), ALL, 0)]
    exp = [model(r, *q) for r, q in zip(refs, queries)]
    errors = []

    def work(j):
        try:
            flt, order, k = queries[j]
            for _ in range(3):
                got = sa.repeated_substrings(refs[j][0], *flt, order=order, k=k)
                st = sa.last_substr_stats()
                assert np.array_equal(got, exp[j][0])
                check_stats(refs[j], flt, order, k, st)
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
