"""CPU suite for document collections over the token indexes (include/sa_amd_tokdocs.h): the header and
the two libraries, the definitions -- doc_of, occ, df, the listing in slot order, the Boolean R(q) and the offsets a separator
token gives -- restated in numpy over the token definitions of tests/test_tokens_abi.py and checked against literal brute force,
the header's example, the Python surface, and the argument checks that answer without a device.  tests/test_token_docs.py and
tests/test_token_docs_guards.py import the definitions from here."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import Not
from conftest import ROOT
import test_streams
from test_tokens_abi import brute_suffix_array, range_definition

OPS = ("set_documents", "set_documents_by_separator", "doc_offsets", "doc_of", "doc_search", "doc_list", "doc_match", "doc_match_list")
PREFIXES = {16: "sa_amd_tok_index_", 32: "sa_amd_tok32_index_"}
DTYPES = {16: np.uint16, 32: np.uint32}
EXPORTS = tuple(p + op for p in PREFIXES.values() for op in OPS)
HEADER = "sa_amd_tokdocs.h"
EINVAL, ERANGE, DOC_NONE = -1, -6, 0xFFFFFFFF
LIMIT = {16: 1 << 16, 32: 1 << 24}                                    # the first id that is no token
A, B, C, D, R = 0x00FF, 0x0100, 0x01FF, 0x0200, 0xFF00                # the header's ids of a, b, c, d, r
LETTER = {"a": A, "b": B, "c": C, "d": D, "r": R}
EXAMPLE_OFF = [0, 4, 4, 7, 11]


def word(s):
    """a string over the header's letters -> its token ids"""
    return [LETTER[ch] for ch in s]


EXAMPLE_TEXT = word("abracadabra")


# ---------------------------------------------------------------- the definitions ----

def separator_offsets(tokens, sep):
    """the collection sa_amd_tok_index_set_documents_by_separator defines: the issue's numpy expression"""
    T = np.asarray(tokens)
    n = T.size
    return np.concatenate(([0], np.flatnonzero(T == sep) + 1, [n] if n == 0 or T[-1] != sep else [])).astype(np.uint32)


def doc_of_definition(off, n, pos):
    """doc(p): the d with off[d] <= p < off[d + 1]; DOC_NONE for p >= n"""
    off, pos = np.asarray(off, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    d = np.searchsorted(off, pos, "right") - 1
    return np.where(pos >= n, DOC_NONE, d).astype(np.uint32)


def answers_definition(t, off, arr, pats):
    """-> (occ, df, the listings in slot order) of token patterns: t the text as a list of ints, arr its token suffix array.  occ
    is hi - lo of the token search; the empty suffix (slot 0) belongs to no document."""
    n = len(t)
    occ, df, lists = [], [], []
    for p in pats:
        lo, hi = range_definition(t, arr, [int(x) for x in p])
        starts = np.array([arr[i] for i in range(lo, hi) if arr[i] < n], dtype=np.int64)
        docs = doc_of_definition(off, n, starts).astype(np.int64)
        _, first = np.unique(docs, return_index=True)
        listing = docs[np.sort(first)]
        occ.append(hi - lo)
        df.append(listing.size)
        lists.append(listing)
    return np.array(occ, dtype=np.int64), np.array(df, dtype=np.int64), lists


def is_pattern(x):
    return sa._is_token_pattern(x)


def clauses_of(query):
    """a query of the Python surface -> [(patterns as tuples of ints, negated)]"""
    out = []
    for clause in query:
        neg = isinstance(clause, Not)
        body = clause.clause if neg else clause
        pats = [body] if is_pattern(body) else list(body)
        out.append(([tuple(int(x) for x in p) for p in pats], neg))
    return out


def match_definition(t, off, arr, queries):
    """-> (df per query, clause_df per clause in the order given, the listings: ascending document ids): U(c) the union of
    D(p), S(c) = U or its complement, R(q) the intersection -- include/suffix_array_amd_docmatch.h over token patterns"""
    ndocs = len(off) - 1
    everything = set(range(ndocs))
    uniq = sorted({p for q in queries for pats, _ in clauses_of(q) for p in pats})
    lists = answers_definition(t, off, arr, uniq)[2] if uniq else []
    Dp = {p: set(int(d) for d in l) for p, l in zip(uniq, lists)}
    df, cdf, listings = [], [], []
    for q in queries:
        Rq = set(everything)
        for pats, neg in clauses_of(q):
            U = set().union(*[Dp[p] for p in pats]) if pats else set()
            S = everything - U if neg else U
            cdf.append(len(S))
            Rq &= S
        df.append(len(Rq))
        listings.append(np.array(sorted(Rq), dtype=np.int64))
    return np.array(df, dtype=np.int64), np.array(cdf, dtype=np.int64), listings


# ---------------------------------------------------------------- brute force ----

def brute_starts(t, pat):
    """every position where pat starts, the empty suffix's n included for the empty pattern"""
    p = len(pat)
    return [i for i in range(len(t) + 1) if t[i:i + p] == list(pat)]


def brute_docs(t, off, pat):
    """D(p) by looking at every start: a linear search for the document"""
    n, out = len(t), set()
    for s in brute_starts(t, pat):
        if s < n:
            out.add(max(d for d in range(len(off) - 1) if off[d] <= s))
    return out


def brute_match(t, off, queries):
    ndocs = len(off) - 1
    df, cdf, listings = [], [], []
    for q in queries:
        Rq = set(range(ndocs))
        for pats, neg in clauses_of(q):
            U = set()
            for p in pats:
                U |= brute_docs(t, off, p)
            S = set(range(ndocs)) - U if neg else U
            cdf.append(len(S))
            Rq &= S
        df.append(len(Rq))
        listings.append(sorted(Rq))
    return df, cdf, listings


def random_offsets(n, ndocs, rng):
    """ndocs + 1 offsets with random cuts; equal neighbours are empty documents"""
    cuts = np.sort(rng.integers(0, n + 1, ndocs - 1)) if ndocs > 1 else np.zeros(0, dtype=np.int64)
    return np.concatenate(([0], cuts, [n])).astype(np.int64)


def patterns_of(t, rng, alphabet):
    """substrings of the text, absent ones, the empty pattern and the whole text"""
    n = len(t)
    pats = [[], list(t), list(t) + [alphabet[0]]]
    for k in (1, 1, 2, 2, 3, 5):
        if n >= k:
            a = int(rng.integers(0, n - k + 1))
            pats.append(list(t[a:a + k]))
        pats.append([int(alphabet[int(rng.integers(0, len(alphabet)))]) for _ in range(k)])
    return pats


def queries_of(pats, rng):
    """the shapes of query of tests/test_doc_match_abi.py over token patterns (the empty pattern is an empty array: an empty
    list is a clause without patterns)"""
    def pick():
        return pats[int(rng.integers(0, len(pats)))] or EMPTY
    a, b, c, d = pick(), pick(), pick(), pick()
    out = [[], [[]], [Not([])], [[], a], [a], [Not(a)], [a, b], [a, Not(b)], [Not(a), Not(b)], [[a, a]], [a, Not(a)],
           [[a, b], Not([c, d])], [[a, b, c, d]], [EMPTY], [Not(EMPTY)], [[EMPTY, a], Not(b)],
           [[pick(), pick()] if k % 2 else Not(pick()) for k in range(9)]]
    for _ in range(3):
        out.append([[pick() for _ in range(int(rng.integers(0, 4)))] if rng.random() < 0.6 else Not(pick())
                    for _ in range(int(rng.integers(0, 5)))])
    return out


EMPTY = np.zeros(0, dtype=np.int64)


def test_definitions_against_brute_force_on_random_tiny_texts():
    rng = np.random.default_rng(2027)
    seen = 0
    for case in range(60):
        n = int(rng.integers(0, 41))
        alphabet = [A, B, R, 0xFFFF][:int(rng.integers(1, 5))]
        t = [int(alphabet[int(x)]) for x in rng.integers(0, len(alphabet), n)]
        arr = brute_suffix_array(t).tolist()
        off = random_offsets(n, int(rng.integers(1, 8)), rng)
        pats = patterns_of(t, rng, alphabet)
        occ, df, lists = answers_definition(t, off, arr, pats)
        for q, p in enumerate(pats):
            starts = brute_starts(t, p)
            assert occ[q] == len(starts), (case, p)
            assert set(lists[q].tolist()) == brute_docs(t, off, p) and df[q] == len(lists[q]) == len(set(lists[q].tolist())), (case, p)
        assert occ[0] == n + 1 and df[0] == np.count_nonzero(np.diff(off))      # the empty pattern: the non-empty documents
        pos = np.concatenate((np.arange(n + 3), [DOC_NONE]))
        want = [DOC_NONE if p >= n else max(d for d in range(len(off) - 1) if off[d] <= p) for p in pos.tolist()]
        assert doc_of_definition(off, n, pos).tolist() == want, case
        queries = queries_of(pats, rng)
        got = match_definition(t, off, arr, queries)
        bdf, bcdf, blists = brute_match(t, off, queries)
        assert got[0].tolist() == bdf and got[1].tolist() == bcdf and [l.tolist() for l in got[2]] == blists, case
        sep = int(alphabet[0])
        so = separator_offsets(t, sep)                                  # the separator's collection, by a loop
        ends = [i + 1 for i, x in enumerate(t) if x == sep]
        assert so.tolist() == [0] + ends + ([n] if n == 0 or t[-1] != sep else []), case
        assert so[-1] == n and np.all(np.diff(so.astype(np.int64)) >= (0 if n == 0 else 1)), case     # never an empty document
        seen += 1
    assert seen == 60


def header_text(name=HEADER):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def declarations():
    plain = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    return {fn: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
            for fn, params in re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", plain)}


def test_the_header_example():
    """the values of the two byte headers, on the token text; the literal lines stand in the header"""
    t, off = EXAMPLE_TEXT, EXAMPLE_OFF
    arr = brute_suffix_array(t).tolist()
    assert arr == [11, 10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2]              # the byte text's array: the ids compare as the letters do
    le = sorted(range(12), key=lambda i: [((x & 0xFF) << 8) | (x >> 8) for x in t[i:]])
    assert le != arr                                                  # ... and their little-endian bytes do not
    occ, df, lists = answers_definition(t, off, arr, [word("a"), word("bra"), []])
    assert occ.tolist() == [5, 2, 12] and df.tolist() == [3, 2, 3]
    assert lists[0].tolist() == [3, 0, 2] and lists[1].tolist() == [3, 0]
    a, bra, c, ac = word("a"), word("bra"), word("c"), word("ac")
    queries = [[a, bra], [a, Not(bra)], [Not(a)], [[c, bra]], [ac], [a, c, bra], []]
    mdf, _, mlists = match_definition(t, off, arr, queries)
    assert mdf.tolist() == [2, 1, 1, 3, 1, 0, 4]
    assert [l.tolist() for l in mlists] == [[0, 3], [2], [1], [0, 2, 3], [0], [], [0, 1, 2, 3]]
    assert brute_match(t, off, queries) == (mdf.tolist(), match_definition(t, off, arr, queries)[1].tolist(), [l.tolist() for l in mlists])
    assert doc_of_definition(off, 11, [0, 3, 4, 6, 7, 10, 11]).tolist() == [0, 0, 2, 2, 3, 3, DOC_NONE]
    header = re.sub(r"\s*\n \*\s*", " ", header_text())
    for line in ('T = "abracadabra" with a = 0x00ff, b = 0x0100, c = 0x01ff, d = 0x0200, r = 0xff00',
                 "doc_off = {0, 4, 4, 7, 11}", '"a" has occ 5, df 3 and the listing {3, 0, 2}', '"bra" has occ 2, df 2, listing {3, 0}',
                 '"" has df 3', "a AND bra {0, 3} 2", "a AND NOT bra {2} 1", "NOT a {1} 1", "(c OR bra) {0, 2, 3} 3", "ac {0} 1",
                 "a AND c AND bra {} 0", "no clauses {0, 1, 2, 3} 4", "the threading rule of sa_amd_index_set_documents"):
        assert line in re.sub(r" +", " ", header), line


def test_header_declares_and_both_libraries_export_the_sixteen_functions():
    header, decls = header_text(), declarations()
    assert set(decls) == set(EXPORTS) and len(decls) == 16
    for fn, params in decls.items():
        assert not any("stream" in p for p in params) and not fn.endswith("_device"), fn
    for path in (sa.library_path(), os.path.join(os.path.dirname(sa.library_path()), "libsuffix_array_amd_diag.so")):
        L = ctypes.CDLL(path)
        for fn in EXPORTS:
            assert hasattr(L, fn), (path, fn)
    main = header_text("suffix_array_amd.h")
    assert HEADER not in main and re.search(r'^#include "suffix_array_amd.h"$', header, re.M)
    assert not re.fullmatch(r"suffix_array_amd(_\w+)?\.h", HEADER)
    assert sorted(test_streams.interface_headers()) == ["suffix_array_amd.h", "suffix_array_amd_docmatch.h", "suffix_array_amd_tok32.h"]
    for op in OPS:                                                    # the 32-bit form is the 16-bit one with its own handle and uint32_t patterns
        p16, p32 = decls[PREFIXES[16] + op], decls[PREFIXES[32] + op]
        assert [p.replace("sa_amd_tok_index", "sa_amd_tok32_index").replace("const uint16_t *pat_data", "const uint32_t *pat_data") for p in p16] == p32
    byte = test_streams.interface_headers()
    plain = "\n".join(byte.values())
    bdecl = {fn: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
             for fn, params in re.findall(r"\b(sa_amd_index_\w+)\s*\(([^;{}()]*)\)\s*;", plain)}
    for op in ("set_documents", "doc_of", "doc_search", "doc_list", "doc_match", "doc_match_list"):       # the parameters of the byte forms
        want = [p.replace("sa_amd_index", "sa_amd_tok_index").replace("const uint8_t *pat_data", "const uint16_t *pat_data")
                for p in bdecl["sa_amd_index_" + op]]
        assert decls[PREFIXES[16] + op] == want, op
    assert decls[PREFIXES[16] + "set_documents_by_separator"] == ["sa_amd_tok_index *ix", "uint32_t separator", "int64_t *ndocs_out"]
    assert decls[PREFIXES[16] + "doc_offsets"] == ["const sa_amd_tok_index *ix", "uint32_t *doc_off_out", "int64_t capacity", "int64_t *ndocs_out"]
    probe = ("int32_t (*probe)(sa_amd_tok32_index *, uint32_t, int64_t *) = sa_amd_tok32_index_set_documents_by_separator;\n"
             "int32_t (*probe2)(const sa_amd_tok_index *, const uint16_t *, const int64_t *, int32_t, uint32_t *, uint32_t *) = sa_amd_tok_index_doc_search;\n")
    for first in ("#include \"sa_amd_tokdocs.h\"\n", "#include \"suffix_array_amd.h\"\n#include \"sa_amd_tokdocs.h\"\n"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=(first + probe).encode(), check=True)


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert sa.TOKEN_DOC_OPS == OPS
    for cls in (sa.TokenIndex, sa.TokenIndex32):
        sig = inspect.signature(cls.set_documents)
        assert list(sig.parameters) == ["self", "offsets", "separator"]
        assert sig.parameters["offsets"].default is None and sig.parameters["separator"].kind is inspect.Parameter.KEYWORD_ONLY
        assert isinstance(cls.ndocs, property)
        assert params(cls.doc_offsets) == ["self"] and params(cls.doc_of) == ["self", "positions"]
        assert params(cls.doc_search) == params(cls.doc_list) == ["self", "patterns"]
        assert params(cls.doc_match) == ["self", "queries", "clause_df"] and params(cls.doc_match_list) == ["self", "queries"]
        assert inspect.signature(cls.doc_match).parameters["clause_df"].default is False
    L = sa.lib()
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    for prefix in PREFIXES.values():
        assert getattr(L, prefix + "set_documents").argtypes == [vp, vp, i64]
        assert getattr(L, prefix + "set_documents_by_separator").argtypes == [vp, u32, vp]
        assert getattr(L, prefix + "doc_offsets").argtypes == [vp, vp, i64, vp]
        assert getattr(L, prefix + "doc_of").argtypes == [vp, vp, i64, vp]
        assert getattr(L, prefix + "doc_search").argtypes == [vp, vp, vp, i32, vp, vp]
        assert getattr(L, prefix + "doc_list").argtypes == [vp, vp, vp, i32, vp, vp, i64, vp]
        assert getattr(L, prefix + "doc_match").argtypes == [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp]
        assert getattr(L, prefix + "doc_match_list").argtypes == [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, i64, vp]
        for op in OPS:
            assert getattr(L, prefix + op).restype is i32
    # the packing helper on token queries: a list of ints is ONE pattern, an empty list a clause without patterns
    q = [[word("a"), Not(word("bra"))], [], [[word("c"), np.array(word("bra"), dtype=np.uint16)], Not([])], [np.zeros(0, dtype=np.uint16)]]
    data, off, npat, coff, cfl, ncl, qoff, nq = sa._query_batch(q, sa._is_token_pattern, lambda p: p, sa._token_batch)
    assert (npat, ncl, nq) == (5, 5, 4) and data.dtype == np.uint16
    assert data[:off[-1]].tolist() == word("abracbra") and off.tolist() == [0, 1, 4, 5, 8, 8]
    assert coff.tolist() == [0, 1, 2, 4, 4, 5] and cfl[:ncl].tolist() == [0, 1, 0, 1, 0] and qoff.tolist() == [0, 2, 2, 4, 5]
    for bad in ([word("a")], [Not(word("a"))]):                       # a query is a sequence of clauses, not a clause
        with pytest.raises(TypeError):
            sa._query_batch(bad, sa._is_token_pattern, lambda p: p, sa._token_batch)
    with pytest.raises(ValueError):                                   # an id of 2^24 in a 32-bit pattern: before the library is called
        sa._token_batch32([[1 << 24]])


def test_cpp_token_indexes_have_the_methods():
    """include/suffix_array_amd.hpp: both token index classes instantiate the document methods, over BasicClause<Tokens>; the
    byte Clause is the same template over std::string"""
    src = ('#include "suffix_array_amd.hpp"\n#include <type_traits>\nusing namespace suffix_array;\n'
           "static_assert(std::is_same<Clause, BasicClause<std::string>>::value, \"\");\n"
           "template <class Ix> std::size_t use(Ix &ix, typename Ix::Token sep) {\n"
           "    using Tokens = typename Ix::Tokens;\n    using C = typename Ix::Clause;\n"
           "    std::size_t s = ix.set_documents({0, 1, 3}) + ix.set_documents_by_separator(sep) + ix.ndocs();\n"
           "    s += ix.doc_offsets().size() + ix.doc_of({0, 1}).size() + ix.doc_search({Tokens{1}, Tokens{2, 3}}).size();\n"
           "    s += ix.doc_list({Tokens{1}}).size() + ix.match({ { C{{Tokens{1}}, false}, C{{Tokens{2, 3}, Tokens{9}}, true} }, {} }).size();\n"
           "    return s + ix.match_list({ { C{} } }).size();\n}\n"
           "template std::size_t use<TokenIndex>(TokenIndex &, std::uint16_t);\n"
           "template std::size_t use<TokenIndex32>(TokenIndex32 &, std::uint32_t);\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)


@pytest.mark.parametrize("width", [16, 32])
def test_argument_checks_answer_without_a_device(width):
    L = sa.lib()
    fn = {op: getattr(L, PREFIXES[width] + op) for op in OPS}
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    small = np.array([1, 2, 3, 4], dtype=DTYPES[width])
    pd = small.ctypes.data
    pat_off = np.array([0, 2, 4], dtype=np.int64)                     # two patterns,
    pat = pat_off.ctypes.data
    good_c = np.array([0, 1, 2], dtype=np.int32)                      # one in each of two clauses,
    good_q = np.array([0, 2], dtype=np.int32)                         # one query
    flags = np.array([0, 1, 0, 0], dtype=np.uint8)
    gc_, gq, fl = good_c.ctypes.data, good_q.ctypes.data, flags.ctypes.data
    before = (sa.last_docs_stats(), sa.last_doc_match_stats())
    good_off = np.array([0, 2, 5], dtype=np.uint32)

    # NULL index, every call
    assert fn["set_documents"](None, good_off.ctypes.data, 2) == EINVAL
    assert fn["set_documents_by_separator"](None, 1, c) == EINVAL
    assert fn["doc_offsets"](None, p, 4, c) == EINVAL
    assert fn["doc_of"](None, p, 4, p) == EINVAL
    assert fn["doc_search"](None, pd, pat, 2, p, p) == EINVAL
    assert fn["doc_list"](None, pd, pat, 2, p, p, 4, c) == EINVAL
    assert fn["doc_match"](None, pd, pat, 2, gc_, fl, 2, gq, 1, p, p) == EINVAL
    assert fn["doc_match_list"](None, pd, pat, 2, gc_, fl, 2, gq, 1, p, p, 4, c) == EINVAL
    # malformed offsets: NULL, no document, a first entry that is not 0, a decrease
    assert fn["set_documents"](fake, None, 2) == EINVAL
    assert fn["set_documents"](fake, good_off.ctypes.data, 0) == EINVAL
    assert fn["set_documents"](fake, good_off.ctypes.data, -1) == EINVAL
    for off in ([1, 2, 5], [0, 3, 2], [0, 5, 4]):
        keep = np.array(off, dtype=np.uint32)
        assert fn["set_documents"](fake, keep.ctypes.data, 2) == EINVAL, off
    # a separator that is no token
    for sep in (LIMIT[width], LIMIT[width] + 1, 0xFFFFFFFF):
        assert fn["set_documents_by_separator"](fake, sep, c) == ERANGE, sep
    # counts, capacities and NULL outputs
    assert fn["doc_offsets"](fake, p, -1, c) == EINVAL and fn["doc_offsets"](fake, p, 4, None) == EINVAL
    assert fn["doc_offsets"](fake, None, 4, c) == EINVAL
    assert fn["doc_of"](fake, p, -1, p) == EINVAL and fn["doc_of"](fake, None, 4, p) == EINVAL and fn["doc_of"](fake, p, 4, None) == EINVAL
    assert fn["doc_search"](fake, pd, pat, -1, p, p) == EINVAL and fn["doc_search"](fake, None, pat, 2, p, p) == EINVAL
    assert fn["doc_search"](fake, pd, None, 2, p, p) == EINVAL
    for off in ([0, 3, 2], [-1, 2, 4], [0, 2, -4]):
        keep = np.array(off, dtype=np.int64)                          # (alive over the calls: .ctypes.data alone does not hold it)
        bad = keep.ctypes.data
        assert fn["doc_search"](fake, pd, bad, 2, p, p) == EINVAL and fn["doc_list"](fake, pd, bad, 2, p, p, 4, c) == EINVAL, off
    assert fn["doc_list"](fake, pd, pat, 2, p, p, -1, c) == EINVAL and fn["doc_list"](fake, pd, pat, 2, None, p, 4, c) == EINVAL
    assert fn["doc_list"](fake, pd, pat, 2, p, p, 4, None) == EINVAL and fn["doc_list"](fake, pd, pat, 2, p, None, 4, c) == EINVAL

    def both(pd_, po, npat, co, cf, ncl, qo, nq):
        return (fn["doc_match"](fake, pd_, po, npat, co, cf, ncl, qo, nq, p, p), fn["doc_match_list"](fake, pd_, po, npat, co, cf, ncl, qo, nq, p, p, 4, c))
    for npat, ncl, nq in ((-1, 2, 1), (2, -1, 1), (2, 2, -1)):
        assert both(pd, pat, npat, gc_, fl, ncl, gq, nq) == (EINVAL, EINVAL)
    assert both(pd, None, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL) and both(None, pat, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL)
    assert both(pd, pat, 2, None, fl, 2, gq, 1) == (EINVAL, EINVAL)                              # malformed clause_off
    for off in ([1, 1, 2], [0, 2, 1], [0, 1, 1], [0, 1, 3], [0, -1, 2]):
        keep = np.array(off, dtype=np.int32)
        assert both(pd, pat, 2, keep.ctypes.data, fl, 2, gq, 1) == (EINVAL, EINVAL), off
    assert both(pd, pat, 2, gc_, fl, 2, None, 1) == (EINVAL, EINVAL)                             # malformed query_off
    for off in ([1, 2], [0, 1], [0, 3], [0, -2]):
        keep = np.array(off, dtype=np.int32)
        assert both(pd, pat, 2, gc_, fl, 2, keep.ctypes.data, 1) == (EINVAL, EINVAL), off
    bad_flags = np.array([0, 2, 0, 0], dtype=np.uint8)
    assert both(pd, pat, 2, gc_, bad_flags.ctypes.data, 2, gq, 1) == (EINVAL, EINVAL)           # unknown flag bits
    lst = fn["doc_match_list"]
    assert lst(fake, pd, pat, 2, gc_, fl, 2, gq, 1, p, p, -1, c) == EINVAL and lst(fake, pd, pat, 2, gc_, fl, 2, gq, 1, None, p, 4, c) == EINVAL
    assert lst(fake, pd, pat, 2, gc_, fl, 2, gq, 1, p, p, 4, None) == EINVAL and lst(fake, pd, pat, 2, gc_, fl, 2, gq, 1, p, None, 4, c) == EINVAL
    # a pattern id that is no token (the 32-bit index only: every 16-bit value is a token), found before the index is used
    if width == 32:
        for at in (0, 3):
            ids = np.array([1, 2, 3, 4], dtype=np.uint32)
            ids[at] = 1 << 24
            assert fn["doc_search"](fake, ids.ctypes.data, pat, 2, p, p) == ERANGE and fn["doc_list"](fake, ids.ctypes.data, pat, 2, p, p, 4, c) == ERANGE
            assert both(ids.ctypes.data, pat, 2, gc_, fl, 2, gq, 1) == (ERANGE, ERANGE)
    assert tot.value == -5 and np.all(buf == 0x77777777)              # nothing was written
    assert (sa.last_docs_stats(), sa.last_doc_match_stats()) == before            # a rejected call leaves the statistics alone
