"""CPU suite for per-document term frequencies and top-k documents: the definitions of include/suffix_array_amd.h (tf, the
slots-by-document table and its two lower bounds, the top-k order) restated in numpy over the oracle's suffix array and checked
against literal brute force; a pure-Python model of the piecewise reduction against the full sort; the exports, the Python
surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases
from test_docs_abi import (EXAMPLE_OFF, EXAMPLE_TEXT, NONE, _u8, brute_starts, brute_suffix_rank, doc_of_definition, listing_definition,
                           offset_tables, patterns_of, range_definition)

EXPORTS = ("sa_amd_index_enable_doc_freq", "sa_amd_index_doc_tf", "sa_amd_index_doc_topk", "sa_amd_last_doc_tf_stats",
           "sa_amd_docs_set_topk_piece")
STATS_FIELDS = ("patterns", "occ_sum", "df_sum", "tf_sum", "table_loads", "topk_entries", "pieces", "rounds", "k", "piece", "chunk",
                "readbacks", "reserved")
ALL_ONES = (1 << 64) - 1


# ---------------------------------------------------------------- the definitions ----

def tf_definition(doc_off, n, arr, lo, hi):
    """-> (the listing, tf next to every document): tf(d) = the slots of [lo, hi) with SA[i] < n and doc(SA[i]) = d"""
    d = doc_of_definition(doc_off, n, np.asarray(arr[lo:hi], dtype=np.int64))
    d = d[d != NONE]
    uniq, first, counts = np.unique(d, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")                          # the order of the slot of the first occurrence
    return uniq[order].astype(np.int64), counts[order].astype(np.int64)


def slots_definition(doc_off, n, arr):
    """S: the slots 1 .. n ordered by document, ascending inside a document"""
    da = doc_of_definition(doc_off, n, np.asarray(arr[1:], dtype=np.int64))
    return np.argsort(da, kind="stable").astype(np.int64) + 1


def tf_by_table(doc_off, S, lo, hi, d):
    """tf(d) = lb(S_d, hi) - lb(S_d, lo) with S_d = S[doc_off[d] .. doc_off[d + 1])"""
    part = S[int(doc_off[d]):int(doc_off[d + 1])]
    return int(np.searchsorted(part, hi, "left") - np.searchsorted(part, lo, "left"))


def topk_definition(docs, tf, k):
    """the min(k, df) documents with the greatest tf, by tf descending and then by document id ascending"""
    docs, tf = np.asarray(docs, dtype=np.int64), np.asarray(tf, dtype=np.int64)
    order = np.lexsort((docs, -tf))[:k]
    return docs[order], tf[order]


def answers_definition(tb, doc_off, arr, pats):
    """-> per pattern (occ, listing, tf)"""
    n = len(tb)
    out = []
    for pat in pats:
        lo, hi = range_definition(tb, arr, pat)
        ls, tf = tf_definition(doc_off, n, arr, lo, hi)
        out.append((hi - lo, ls, tf))
    return out


# ---------------------------------------------------------------- the reduction's model ----

def effective_piece(piece, k):
    """the switch's value (rounded down to a power of two in 64 .. 4096), raised to at least twice the next power of two >= k"""
    p = 1 << (min(max(piece, sa.DOC_TOPK_PIECE_MIN), sa.DOC_TOPK_PIECE_MAX).bit_length() - 1)
    return max(p, 2 * (1 << (k - 1).bit_length()))


def key_of(doc, tf):
    return ((0xFFFFFFFF - int(tf)) << 32) | int(doc)


def reduce_once(keys, P, k):
    """pieces of P keys, each sorted, the first k of each kept -> (the kept keys, the number of pieces)"""
    out, pieces = [], 0
    for a in range(0, len(keys), P):
        out += sorted(keys[a:a + P])[:k]
        pieces += 1
    return out, pieces


def reduction_model(lists, P, k):
    """lists: per pattern its keys in listing order -> (per pattern the top-k keys, rounds, pieces of all rounds).  Every round
    cuts every pattern's list; the round in which no list is longer than P is the last."""
    lists = [list(l) for l in lists]
    rounds = pieces = 0
    while True:
        rounds += 1
        last = all(len(l) <= P for l in lists)
        nxt = []
        for l in lists:
            kept, pc = reduce_once(l, P, k)
            nxt.append(kept)
            pieces += pc
        lists = nxt
        if last:
            return lists, rounds, pieces


def plan_definition(lens, P, k):
    """the same in arithmetic, as a caller who knows list_off can work it out: -> (rounds, pieces, the final lengths)"""
    lens = [int(l) for l in lens]
    rounds = pieces = 0
    while True:
        rounds += 1
        last = all(l <= P for l in lens)
        pieces += sum((l + P - 1) // P for l in lens)
        lens = [(l // P) * k + min(l % P, k) for l in lens]
        if last:
            return rounds, pieces, lens


# ---------------------------------------------------------------- brute force ----

def brute_tf(doc_off, n, starts, k_values=(1, 2, 5)):
    """starts by bytes.find in suffix order -> (listing, tf, {k: ranked (doc, tf) pairs}): the documents in the order the sorted
    starts meet them, the starts counted per document with np.searchsorted, ranked with sorted() on (-tf, doc)"""
    offa = np.asarray(doc_off, dtype=np.int64)
    inside = starts[starts < n]
    d = np.searchsorted(offa, inside, "right") - 1
    ls = list(dict.fromkeys(d.tolist()))
    pos = np.sort(inside)
    tf = [int(np.searchsorted(pos, offa[x + 1], "left") - np.searchsorted(pos, offa[x], "left")) for x in ls]
    ranked = sorted(zip(ls, tf), key=lambda e: (-e[1], e[0]))
    return ls, tf, {k: ranked[:k] for k in k_values}


def _brute_check(tb, oracle, rng, tables=None):
    """every table shape (or `tables`) over one text, the same patterns under each"""
    n = len(tb)
    arr = oracle.sais(_u8(tb))
    rank = brute_suffix_rank(tb)
    pats = patterns_of(tb, rng)
    starts = [brute_starts(tb, pat, rank) for pat in pats]
    for name, off in (tables or offset_tables(n, rng)).items():
        offa = np.asarray(off, dtype=np.int64)
        S = slots_definition(off, n, arr)
        assert S.size == n and sorted(S.tolist()) == list(range(1, n + 1)), name
        for d in range(len(off) - 1):                                 # document d owns S[off[d] .. off[d + 1]), ascending: one slot per position
            part = S[int(offa[d]):int(offa[d + 1])]
            assert np.all(np.diff(part) > 0) and sorted(int(arr[i]) for i in part) == list(range(int(offa[d]), int(offa[d + 1]))), (name, d)
            if d > 40:
                break
        for q, (occ, ls, tf) in enumerate(answers_definition(tb, off, arr, pats)):
            lo, hi = range_definition(tb, arr, pats[q])
            bl, bt, ranked = brute_tf(off, n, starts[q])
            assert np.array_equal(ls, listing_definition(off, n, arr, lo, hi))
            assert (ls.tolist(), tf.tolist()) == (bl, bt), (name, pats[q][:16])
            assert [tf_by_table(offa, S, lo, hi, d) for d in ls] == bt, (name, pats[q][:16])
            assert int(tf.sum()) == occ - (0 if pats[q] else 1)
            for k, want in ranked.items():
                td, tt = topk_definition(ls, tf, k)
                assert list(zip(td.tolist(), tt.tolist())) == want, (name, pats[q][:16], k)
                keys = sorted(key_of(a, b) for a, b in zip(ls, tf))[:k]    # ascending key order is the wanted order
                assert [(x & 0xFFFFFFFF, 0xFFFFFFFF - (x >> 32)) for x in keys] == want
        occ, ls, tf = answers_definition(tb, off, arr, [b""])[0]          # the empty pattern: tf(d) is the length of document d
        assert tf.tolist() == [int(offa[d + 1] - offa[d]) for d in ls]


def test_the_header_example(oracle):
    tb, off = EXAMPLE_TEXT, EXAMPLE_OFF
    arr = oracle.sais(_u8(tb))
    ans = answers_definition(tb, off, arr, [b"a", b"bra", b"", b"zz"])
    assert [(a[1].tolist(), a[2].tolist()) for a in ans] == [([3, 0, 2], [2, 2, 1]), ([3, 0], [1, 1]), ([3, 0, 2], [4, 4, 3]), ([], [])]
    top = {k: list(zip(*[x.tolist() for x in topk_definition(ans[0][1], ans[0][2], k)])) for k in (1, 2, 5)}
    assert top == {1: [(0, 2)], 2: [(0, 2), (3, 2)], 5: [(0, 2), (3, 2), (2, 1)]}
    assert slots_definition(off, 11, arr).tolist() == [3, 4, 7, 11, 5, 8, 9, 1, 2, 6, 10]
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    assert '"a" has the listing {3, 0, 2} with tf {2, 2, 1}; its top-1 is (0, 2), its\n *     top-2 is (0, 2), (3, 2), its top-5 is (0, 2), (3, 2), (2, 1)' in header
    assert '"bra" has tf {1, 1}' in header and 'tf {4, 4, 3}' in header
    _brute_check(tb, oracle, np.random.default_rng(1), {"example": off})


def test_definitions_against_brute_force_random(oracle):
    rng = np.random.default_rng(18)
    for trial in range(40):
        n = int(rng.integers(0, 50))
        sigma = int(rng.choice([1, 2, 3, 4, 26]))
        _brute_check(rng.integers(97, 97 + sigma, n).astype(np.uint8).tobytes(), oracle, rng)


def test_definitions_against_brute_force_golden(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        manifest = json.load(f)
    names = sorted(manifest)
    rng = np.random.default_rng(19)
    for name in names:
        with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
            tb = f.read()
        _brute_check(tb, oracle, rng)                                 # every table shape on every golden text
    assert len(names) >= 5


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_definitions_against_brute_force_adversarial(oracle, name):
    tb = adversarial_cases()[name]
    _brute_check(tb, oracle, np.random.default_rng(len(tb) + 1))


# ---------------------------------------------------------------- the reduction ----

def _tf_shapes(df, rng):
    docs = rng.permutation(4 * df + 7)[:df]                           # distinct ids in listing (not id) order
    return {"equal": (docs, np.full(df, 5)), "distinct": (docs, rng.permutation(df) + 1), "two_values": (docs, rng.integers(1, 3, df))}


@pytest.mark.parametrize("piece", [64, 128, 4096])
@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 1024])
def test_reduction_model_equals_the_full_sort(piece, k):
    P = effective_piece(piece, k)
    assert P >= 2 * k and P >= piece and P & (P - 1) == 0
    rng = np.random.default_rng(piece + k)
    for df in (0, 1, P - 1, P, P + 1, 5 * P, 40 * P):
        for shape, (docs, tf) in _tf_shapes(df, rng).items():
            keys = [key_of(d, t) for d, t in zip(docs.tolist(), tf.tolist())]
            assert len(set(keys)) == df and all(x < ALL_ONES for x in keys)      # distinct inside a pattern, below the padding
            (got,), rounds, pieces = reduction_model([keys], P, k)
            td, tt = topk_definition(docs, tf, k)
            assert got == [key_of(d, t) for d, t in zip(td.tolist(), tt.tolist())], (df, shape)
            assert (rounds, pieces, [len(got)]) == plan_definition([df], P, k) and (rounds == 1) == (df <= P)


def test_reduction_model_rounds_and_mixed_batches():
    """every round at least halves a list longer than P; a batch ends with its longest list"""
    rng = np.random.default_rng(3)
    for P, k in ((64, 16), (64, 32), (128, 1), (128, 64)):
        for df in (P + 1, 2 * P, 40 * P, 40 * P + 1):
            docs, tf = _tf_shapes(df, rng)["two_values"]
            cur = [key_of(d, t) for d, t in zip(docs.tolist(), tf.tolist())]
            while len(cur) > P:
                nxt, _ = reduce_once(cur, P, k)
                assert len(nxt) <= (len(cur) + P) // 2 and len(nxt) < len(cur)
                cur = nxt
    lists = []
    for df in (0, 1, 3000, 0, 64, 65):
        docs, tf = _tf_shapes(df, rng)["distinct"]
        lists.append([key_of(d, t) for d, t in zip(docs.tolist(), tf.tolist())])
    got, rounds, pieces = reduction_model(lists, 64, 16)
    assert [len(g) for g in got] == [0, 1, 16, 0, 16, 16] and all(g == sorted(l)[:16] for g, l in zip(got, lists))
    assert (rounds, pieces) == plan_definition([len(l) for l in lists], 64, 16)[:2]
    assert rounds == reduction_model([lists[2]], 64, 16)[1] >= 3      # 3000 -> 47 pieces -> 752 keys -> 12 pieces -> 192 -> 3 -> 48 -> 1


# ---------------------------------------------------------------- the surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_DOC_TOPK_MAX\s+1024\b", header) and sa.DOC_TOPK_MAX == 1024
    body = header[header.index("typedef struct sa_amd_doc_tf_stats"):header.index("} sa_amd_doc_tf_stats;")]
    declared = re.findall(r"^\s+int(64|32)_t\s+(\w+);", body, re.M)
    assert [name for _, name in declared] == list(STATS_FIELDS) == [name for name, _ in sa.DocTfStats._fields_]
    for (bits, name), (_, ctype) in zip(declared, sa.DocTfStats._fields_):
        assert ctypes.sizeof(ctype) * 8 == int(bits), name
    assert ctypes.sizeof(sa.DocTfStats) == 7 * 8 + 6 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "doc_tf.hpp")) as f:
        kernels = f.read()
    for name in ("DOC_TOPK_MAX", "DOC_TOPK_PIECE_MIN", "DOC_TOPK_PIECE_MAX", "DOC_TOPK_PIECE_DEFAULT"):
        m = re.search(r"constexpr int " + name + r" = ([^;]+);", kernels)
        assert m and eval(m.group(1)) == getattr(sa, name), name      # noqa: S307 (an integer expression of the project's own source)
    assert (sa.DOC_TOPK_PIECE_MIN, sa.DOC_TOPK_PIECE_MAX, sa.DOC_TOPK_PIECE_DEFAULT) == (64, 4096, 1024)


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.enable_doc_freq) == ["self"]
        assert params(cls.doc_tf) == ["self", "patterns"]
        assert params(cls.doc_topk) == ["self", "patterns", "k"]
    assert params(sa.docs_set_topk_piece) == ["entries"] and params(sa.last_doc_tf_stats) == []
    for name in ("DocTfStats", "last_doc_tf_stats", "docs_set_topk_piece", "DOC_TOPK_MAX", "DOC_TOPK_PIECE_MIN", "DOC_TOPK_PIECE_MAX",
                 "DOC_TOPK_PIECE_DEFAULT"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert set(sa.last_doc_tf_stats()) == set(STATS_FIELDS) - {"reserved"}


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    assert L.sa_amd_index_enable_doc_freq(None) == -1                                           # NULL index
    assert L.sa_amd_index_doc_tf(None, p, good.ctypes.data, 2, p, p, p, 4, c) == -1
    assert L.sa_amd_index_doc_topk(None, p, good.ctypes.data, 2, 3, p, p, p) == -1
    for k in (0, -1, sa.DOC_TOPK_MAX + 1, 2**31 - 1):                                           # k out of range
        assert L.sa_amd_index_doc_topk(fake, p, good.ctypes.data, 2, k, p, p, p) == -1
    assert L.sa_amd_index_doc_tf(fake, p, good.ctypes.data, -1, p, p, p, 4, c) == -1            # negative count, capacity
    assert L.sa_amd_index_doc_tf(fake, p, good.ctypes.data, 2, p, p, p, -1, c) == -1
    assert L.sa_amd_index_doc_topk(fake, p, good.ctypes.data, -1, 3, p, p, p) == -1
    assert L.sa_amd_index_doc_tf(fake, p, good.ctypes.data, 2, None, p, p, 4, c) == -1          # NULL list_off, total_out, top_off
    assert L.sa_amd_index_doc_tf(fake, p, good.ctypes.data, 2, p, p, p, 4, None) == -1
    assert L.sa_amd_index_doc_topk(fake, p, good.ctypes.data, 2, 3, None, p, p) == -1
    for off in bad:                                                                              # pat_off as sa_amd_index_search rejects it
        assert L.sa_amd_index_doc_tf(fake, p, off.ctypes.data, 2, p, p, p, 4, c) == -1
        assert L.sa_amd_index_doc_topk(fake, p, off.ctypes.data, 2, 3, p, p, p) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777)
    L.sa_amd_last_doc_tf_stats(None)


def test_piece_switch():
    try:
        assert sa.docs_set_topk_piece(100) == sa.DOC_TOPK_PIECE_DEFAULT
        assert sa.docs_set_topk_piece(0) == 64                         # rounded down to a power of two
        assert sa.docs_set_topk_piece(1 << 30) == sa.DOC_TOPK_PIECE_MIN
        assert sa.docs_set_topk_piece(2047) == sa.DOC_TOPK_PIECE_MAX
        assert sa.docs_set_topk_piece(-1) == 1024
        assert sa.docs_set_topk_piece(-7) == sa.DOC_TOPK_PIECE_DEFAULT
    finally:
        sa.docs_set_topk_piece(-1)
    for piece, k, want in ((64, 1, 64), (64, 16, 64), (64, 32, 64), (64, 33, 128), (100, 1, 64), (4096, 1024, 4096), (64, 1024, 2048), (128, 31, 128)):
        assert effective_piece(piece, k) == want
