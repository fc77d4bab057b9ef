"""CPU suite for Boolean document queries (include/suffix_array_amd_docmatch.h): the definitions -- D(p),
the clause sets with OR and NOT, the query's intersection, df, clause_df and the ascending listing -- restated with Python sets
over answers_definition of tests/test_docs_abi.py and checked against literal brute force; a model of the statistics (marks,
units, bitmap words, slabs); the header, the exports, the Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import Not
from conftest import ROOT, adversarial_cases
from test_docs_abi import EXAMPLE_OFF, EXAMPLE_TEXT, _u8, answers_definition, offset_tables, patterns_of, units_definition

EXPORTS = ("sa_amd_index_doc_match", "sa_amd_index_doc_match_list", "sa_amd_last_doc_match_stats", "sa_amd_doc_match_set_budget")
STATS_FIELDS = ("patterns", "clauses", "queries", "occ_sum", "units", "marks", "bitmap_words", "slabs", "df_sum", "budget", "chunk",
                "readbacks", "listed")
BUDGET_MIN, BUDGET_MAX = 4096, 1 << 40
EINVAL = -1


# ---------------------------------------------------------------- the definitions ----

def clauses_of(query):
    """a query of the Python surface -> [(patterns, negated)]"""
    out = []
    for clause in query:
        neg = isinstance(clause, Not)
        body = clause.clause if neg else clause
        out.append(([bytes(body)] if isinstance(body, (bytes, bytearray)) else [bytes(p) for p in body], neg))
    return out


def match_definition(tb, off, arr, queries):
    """-> (df per query, clause_df per clause in the order given, the listings: ascending document ids), from D(p) = the listing
    of answers_definition as a set"""
    ndocs = len(off) - 1
    everything = set(range(ndocs))
    flat = [p for q in queries for pats, _ in clauses_of(q) for p in pats]
    uniq = sorted(set(flat))
    _, _, lists = answers_definition(tb, off, arr, uniq) if uniq else (None, None, [])
    D = {p: set(int(d) for d in l) for p, l in zip(uniq, lists)}
    df, cdf, listings = [], [], []
    for q in queries:
        R = set(everything)
        for pats, neg in clauses_of(q):
            U = set().union(*[D[p] for p in pats]) if pats else set()
            S = everything - U if neg else U
            cdf.append(len(S))
            R &= S
        df.append(len(R))
        listings.append(np.array(sorted(R), dtype=np.int64))
    return np.array(df, dtype=np.int64), np.array(cdf, dtype=np.int64), listings


def slabs_definition(clauses_per_query, W, budget):
    """consecutive whole queries while their clauses' bitmaps (4 W bytes each) fit the budget; at least one query a slab"""
    slabs, q, nq = 0, 0, len(clauses_per_query)
    while q < nq:
        rows = clauses_per_query[q]
        q += 1
        while q < nq and (rows + clauses_per_query[q]) * 4 * W <= budget:
            rows += clauses_per_query[q]
            q += 1
        slabs += 1
    return slabs


def stats_definition(tb, off, arr, queries, chunk, budget, listed):
    """every field of sa_amd_doc_match_stats from the inputs"""
    flat = [p for q in queries for pats, _ in clauses_of(q) for p in pats]
    uniq = sorted(set(flat))                                          # (a pattern given twice is searched and marked twice)
    uocc, udf, _ = answers_definition(tb, off, arr, uniq) if uniq else (np.zeros(0, dtype=np.int64),) * 2 + ([],)
    at = {p: k for k, p in enumerate(uniq)}
    pick = np.array([at[p] for p in flat], dtype=np.int64)
    occ, dfp = uocc[pick], udf[pick]
    df, _, _ = match_definition(tb, off, arr, queries)
    W = (len(off) - 1 + 31) // 32
    per_query = [len(q) for q in queries]
    return {"patterns": len(flat), "clauses": sum(per_query), "queries": len(queries), "occ_sum": int(occ.sum()),
            "units": units_definition(occ, chunk), "marks": int(dfp.sum()), "bitmap_words": W,
            "slabs": slabs_definition(per_query, W, budget), "df_sum": int(df.sum()), "budget": budget, "chunk": chunk,
            "readbacks": 1 if flat else 0, "listed": 1 if listed else 0}


# ---------------------------------------------------------------- brute force ----

def brute_docs(tb, off, pat):
    """D(p): bytes.find from every start, np.searchsorted for the document; the empty suffix belongs to no document"""
    n, starts, p = len(tb), [], tb.find(pat)
    while p >= 0:
        starts.append(p)
        p = tb.find(pat, p + 1)
    inside = np.array([s for s in starts if s < n], dtype=np.int64)
    return set((np.searchsorted(np.asarray(off, dtype=np.int64), inside, "right") - 1).tolist())


def brute_match(tb, off, queries):
    ndocs = len(off) - 1
    df, cdf, listings = [], [], []
    for q in queries:
        R = set(range(ndocs))
        for pats, neg in clauses_of(q):
            U = set()
            for p in pats:
                U |= brute_docs(tb, off, p)
            S = set(range(ndocs)) - U if neg else U
            cdf.append(len(S))
            R &= S
        df.append(len(R))
        listings.append(sorted(R))
    return df, cdf, listings


def queries_of(pats, rng):
    """every shape of query over the patterns: no clauses, empty clauses, negated and all-negated ones, a pattern twice in a
    clause, the same pattern in two clauses, the empty pattern, OR of several, many clauses"""
    def pick():
        return pats[int(rng.integers(0, len(pats)))]
    a, b, c, d = pick(), pick(), pick(), pick()
    out = [[], [[]], [Not([])], [[], a], [Not([]), a],
           [a], [Not(a)], [a, b], [a, Not(b)], [Not(a), Not(b)], [Not(a), Not(b), Not(c)],
           [[a, a]], [a, a], [a, Not(a)], [[a, b], Not([c, d])], [[a, b, c, d]], [Not([a, b])],
           [b""], [Not(b"")], [b"", a], [[b"", a], Not(b)],
           [pick() for _ in range(5)], [[pick(), pick()] if k % 2 else Not(pick()) for k in range(16)]]
    for _ in range(6):
        out.append([[pick() for _ in range(int(rng.integers(0, 4)))] if rng.random() < 0.6 else Not(pick())
                    for _ in range(int(rng.integers(0, 5)))])
    return out


def _check_text(tb, oracle, rng, tables=None):
    """the model on every table shape (or `tables`) over one text; against brute force where the text has at most 80 bytes"""
    n = len(tb)
    arr = oracle.sais(_u8(tb))
    pats = patterns_of(tb, rng)
    for name, off in (tables or offset_tables(n, rng)).items():
        queries = queries_of(pats, rng)
        df, cdf, lists = match_definition(tb, off, arr, queries)
        ndocs = len(off) - 1
        assert df[0] == ndocs and df[1] == 0 and df[2] == ndocs, name          # no clauses: all; an empty clause: none; its negation: all
        assert df[17] == np.count_nonzero(np.diff(off)) and df[18] == ndocs - df[17], name     # the empty pattern: the non-empty documents
        assert cdf.size == sum(len(q) for q in queries) and len(lists) == len(queries)
        for q, ls in enumerate(lists):
            assert ls.size == df[q] and np.all(np.diff(ls) > 0), (name, q)
        if n <= 80:
            bdf, bcdf, blists = brute_match(tb, off, queries)
            assert df.tolist() == bdf and cdf.tolist() == bcdf and [l.tolist() for l in lists] == blists, name


def test_the_header_example(oracle):
    tb, off = EXAMPLE_TEXT, EXAMPLE_OFF
    arr = oracle.sais(_u8(tb))
    rows = [([b"a", b"bra"], [0, 3]), ([b"a", Not(b"bra")], [2]), ([Not(b"a")], [1]), ([[b"c", b"bra"]], [0, 2, 3]), ([b"ac"], [0]),
            ([b"a", b"c", b"bra"], []), ([], [0, 1, 2, 3])]
    df, cdf, lists = match_definition(tb, off, arr, [q for q, _ in rows])
    assert [l.tolist() for l in lists] == [want for _, want in rows] and df.tolist() == [2, 1, 1, 3, 1, 0, 4]
    assert cdf.tolist() == [3, 2, 3, 2, 1, 3, 1, 3, 1, 2]
    assert brute_match(tb, off, [q for q, _ in rows])[2] == [want for _, want in rows]
    assert brute_docs(tb, off, b"ac") == {0} and tb.find(b"ac") == 3 and off[1] == 4          # it matches across the boundary at byte 3
    with open(os.path.join(ROOT, "include", "suffix_array_amd_docmatch.h")) as f:
        header = re.sub(r"[ ]+", " ", f.read())
    for line in ("a AND bra {0, 3} 2", "a AND NOT bra {2} 1", "NOT a {1} 1", "(c OR bra) {0, 2, 3} 3", "ac {0} 1", "a AND c AND bra {} 0",
                 "no clauses {0, 1, 2, 3} 4", 'T = "abracadabra", doc_off = {0, 4, 4, 7, 11}'):
        assert line in header, line
    _check_text(tb, oracle, np.random.default_rng(1), {"example": off})
    st = stats_definition(tb, off, arr, [q for q, _ in rows], 64, 4096, False)
    assert st["patterns"] == 11 and st["clauses"] == 10 and st["queries"] == 7 and st["marks"] == (3 + 2) + (3 + 2) + 3 + (1 + 2) + 1 + (3 + 1 + 2)
    assert st["bitmap_words"] == 1 and st["slabs"] == 1 and st["df_sum"] == 12 and st["units"] == 11


def test_a_pattern_that_only_matches_across_a_boundary(oracle):
    tb, off = b"xxabyy" + b"abab", [0, 3, 6, 8, 10]                   # "xxa" "byy" "ab" "ab": "ab" starts in 0 (across), 2 and 3
    arr = oracle.sais(_u8(tb))
    queries = [[b"ab"], [b"ab", Not(b"x")], [b"ayy"], [b"yya"], [Not(b"yya")]]
    df, _, lists = match_definition(tb, off, arr, queries)
    assert [l.tolist() for l in lists] == [[0, 2, 3], [2, 3], [], [1], [0, 2, 3]]
    assert brute_match(tb, off, queries)[2] == [l.tolist() for l in lists]


def test_definitions_against_brute_force_random(oracle):
    rng = np.random.default_rng(26)
    for trial in range(40):
        n = int(rng.integers(0, 60))
        sigma = int(rng.choice([1, 2, 3, 4, 26]))
        _check_text(rng.integers(97, 97 + sigma, n).astype(np.uint8).tobytes(), oracle, rng)


def test_definitions_on_the_golden_texts(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        manifest = json.load(f)
    rng = np.random.default_rng(27)
    for name in sorted(manifest):
        with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
            _check_text(f.read(), oracle, rng)
    assert len(manifest) >= 5


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_definitions_on_the_adversarial_cases(oracle, name):
    tb = adversarial_cases()[name]
    _check_text(tb, oracle, np.random.default_rng(len(tb)))


def test_slabs_model():
    assert slabs_definition([], 1, 4096) == 0
    assert slabs_definition([2] * 10, 1, 4096) == 1
    assert slabs_definition([2] * 10, 512, 4096) == 10                 # 2 clauses * 2 KiB = the budget: one query a slab
    assert slabs_definition([2] * 10, 256, 4096) == 5
    assert slabs_definition([2] * 10, 2048, 4096) == 10                # a query that alone exceeds the budget is a slab of its own
    assert slabs_definition([0] * 7, 2048, 4096) == 1                  # queries without clauses cost nothing
    assert slabs_definition([3, 0, 0, 1, 1, 5], 256, 4096) == 3        # {3, 0, 0, 1} {1} {5}: 4 clauses fit, the fifth does not
    assert slabs_definition([16], 1 << 20, 4096) == 1


# ---------------------------------------------------------------- the surface ----

def header_text(name="suffix_array_amd_docmatch.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def declarations(name="suffix_array_amd_docmatch.h"):
    plain = re.sub(r"/\*.*?\*/", " ", header_text(name), flags=re.S)
    return {fn: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
            for fn, params in re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", plain)}


def test_header_declares_and_library_exports_the_entry_points():
    header, decls = header_text(), declarations()
    assert set(decls) == set(EXPORTS)                                 # what the file declares is what this suite and tests/test_doc_match.py cover
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert hasattr(L, fn), fn
        assert not any("stream" in p for p in decls[fn]), fn         # host pointers only: no device form
    assert not any(fn.endswith("_device") for fn in decls)
    main = header_text("suffix_array_amd.h")
    assert re.search(r'^#include "suffix_array_amd_docmatch.h"$', main, re.M) and re.search(r'^#include "suffix_array_amd.h"$', header, re.M)
    probe = ("#include \"suffix_array_amd.h\"\n"
             "int32_t (*probe)(const sa_amd_index *, const uint8_t *, const int64_t *, int32_t, const int32_t *, const uint8_t *, int32_t,\n"
             "                 const int32_t *, int32_t, uint32_t *, uint32_t *) = sa_amd_index_doc_match;\n"
             "sa_amd_doc_match_stats probe_stats;\n")
    for first in ("", "#include \"suffix_array_amd_docmatch.h\"\n"):                              # either header first
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=(first + probe).encode(), check=True)
    assert decls["sa_amd_index_doc_match_list"][:9] == decls["sa_amd_index_doc_match"][:9]       # the same inputs
    assert decls["sa_amd_index_doc_match_list"][9:] == ["int64_t *list_off", "uint32_t *docs", "int64_t capacity", "int64_t *total_out"]
    body = header[header.index("typedef struct sa_amd_doc_match_stats"):header.index("} sa_amd_doc_match_stats;")]
    fields = re.findall(r"^\s*(int64_t|int32_t)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in sa.DocMatchStats._fields_] == list(STATS_FIELDS) + ["reserved"]
    for (ctype, field), (_, pytype) in zip(fields, sa.DocMatchStats._fields_):
        assert pytype is (ctypes.c_int64 if ctype == "int64_t" else ctypes.c_int32), field
    assert ctypes.sizeof(sa.DocMatchStats) == 10 * 8 + 4 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "host", "doc_match.hpp")) as f:
        host = f.read()
    assert "DM_BUDGET_DEFAULT = (int64_t)256 << 20, DM_BUDGET_MIN = 4096, DM_BUDGET_MAX = (int64_t)1 << 40;" in host
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "doc_match.hpp")) as f:
        kernels = f.read()
    assert "constexpr int DM_LANE_WORDS = 4;" in kernels and "constexpr int DM_TILE_WORDS = WAVE * DM_LANE_WORDS;" in kernels
    assert sa.DOC_MATCH_TILE_WORDS == 64 * 4 and sa.DOC_MATCH_BUDGET_DEFAULT == 256 << 20


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.doc_match) == ["self", "queries", "clause_df"]
        assert inspect.signature(cls.doc_match).parameters["clause_df"].default is False
        assert params(cls.doc_match_list) == ["self", "queries"]
    assert params(sa.doc_match_set_budget) == ["nbytes"] and params(sa.last_doc_match_stats) == []
    for name in ("Not", "DocMatchStats", "last_doc_match_stats", "doc_match_set_budget", "DOC_MATCH_BUDGET_DEFAULT", "DOC_MATCH_TILE_WORDS"):
        assert name in sa.__all__ and hasattr(sa, name), name
    L = sa.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.sa_amd_index_doc_match.argtypes == [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp]
    assert L.sa_amd_index_doc_match_list.argtypes == [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, i64, vp]
    assert L.sa_amd_doc_match_set_budget.argtypes == [i64] and L.sa_amd_doc_match_set_budget.restype is i64
    assert L.sa_amd_last_doc_match_stats.argtypes == [vp]


def test_not_round_trips_through_the_packing_helper():
    queries = [[b"a", Not(b"bra")], [], [[b"c", b"bra"], Not([b"x", b"", b"yy"]), []], [Not([])], ["str", bytearray(b"ba"), _u8(b"np")]]
    data, off, npat, coff, cfl, ncl, qoff, nq = sa._query_batch(queries)
    assert (npat, ncl, nq) == (10, 9, 5)
    assert bytes(data[:off[-1]]) == b"abracbraxyystrbanp" and off.tolist() == [0, 1, 4, 5, 8, 9, 9, 11, 14, 16, 18]
    assert coff.tolist() == [0, 1, 2, 4, 7, 7, 7, 8, 9, 10] and coff.dtype == np.int32
    assert cfl[:ncl].tolist() == [0, 1, 0, 1, 0, 1, 0, 0, 0] and cfl.dtype == np.uint8
    assert qoff.tolist() == [0, 2, 2, 5, 6, 9] and qoff.dtype == np.int32
    back = []                                                         # and back: the same clauses
    for q in range(nq):
        query = []
        for c in range(qoff[q], qoff[q + 1]):
            pats = [bytes(data[off[p]:off[p + 1]]) for p in range(coff[c], coff[c + 1])]
            query.append((pats, bool(cfl[c])))
        back.append(query)
    assert back[:4] == [clauses_of(q) for q in queries[:4]]
    data, off, npat, coff, cfl, ncl, qoff, nq = sa._query_batch([])
    assert (npat, ncl, nq) == (0, 0, 0) and coff.tolist() == [0] and qoff.tolist() == [0] and cfl.size >= 1 and data.size >= 1
    assert repr(Not(b"a")) == "Not(b'a')" and Not([b"a"]).clause == [b"a"]
    for bad in ([b"a"], [Not(b"a")]):                                 # a query is a sequence of clauses, not a clause
        with pytest.raises(TypeError):
            sa._query_batch(bad)
    with pytest.raises(TypeError):
        Not(Not(b"a"))


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    pat = np.array([0, 2, 4], dtype=np.int64).ctypes.data             # two patterns,
    good_c = np.array([0, 1, 2], dtype=np.int32)                      # one in each of two clauses,
    good_q = np.array([0, 2], dtype=np.int32)                         # one query
    flags = np.array([0, 1, 0, 0], dtype=np.uint8)
    gc_, gq, fl = good_c.ctypes.data, good_q.ctypes.data, flags.ctypes.data
    before = sa.last_doc_match_stats()

    def both(ix, pd, po, npat, co, cf, ncl, qo, nq):
        return (L.sa_amd_index_doc_match(ix, pd, po, npat, co, cf, ncl, qo, nq, p, p),
                L.sa_amd_index_doc_match_list(ix, pd, po, npat, co, cf, ncl, qo, nq, p, p, 4, c))
    assert both(None, p, pat, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL)                         # NULL index
    assert both(None, p, pat, 2, gc_, None, 2, gq, 1) == (EINVAL, EINVAL)
    for npat, ncl, nq in ((-1, 2, 1), (2, -1, 1), (2, 2, -1)):                                   # negative counts
        assert both(fake, p, pat, npat, gc_, fl, ncl, gq, nq) == (EINVAL, EINVAL)
    assert both(fake, p, None, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL)                         # pat_off as the search rejects it
    assert both(fake, None, pat, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL)
    for off in ([0, 3, 2], [-1, 2, 4], [0, 2, -4]):
        assert both(fake, p, np.array(off, dtype=np.int64).ctypes.data, 2, gc_, fl, 2, gq, 1) == (EINVAL, EINVAL), off
    assert both(fake, p, pat, 2, None, fl, 2, gq, 1) == (EINVAL, EINVAL)                         # malformed clause_off
    for off in ([1, 1, 2], [0, 2, 1], [0, 1, 1], [0, 1, 3], [0, -1, 2]):
        assert both(fake, p, pat, 2, np.array(off, dtype=np.int32).ctypes.data, fl, 2, gq, 1) == (EINVAL, EINVAL), off
    assert both(fake, p, pat, 2, gc_, fl, 2, None, 1) == (EINVAL, EINVAL)                        # malformed query_off
    for off in ([1, 2], [0, 1], [0, 3], [0, -2]):
        assert both(fake, p, pat, 2, gc_, fl, 2, np.array(off, dtype=np.int32).ctypes.data, 1) == (EINVAL, EINVAL), off
    assert both(fake, p, pat, 2, gc_, fl, 2, np.array([0, 2, 1, 2], dtype=np.int32).ctypes.data, 3) == (EINVAL, EINVAL)
    for bits in (2, 3, 0x80, 0xFF):                                                              # unknown flag bits, in either clause
        for at in (0, 1):
            bad = np.zeros(4, dtype=np.uint8)
            bad[at] = bits
            assert both(fake, p, pat, 2, gc_, bad.ctypes.data, 2, gq, 1) == (EINVAL, EINVAL), (bits, at)
    lst = L.sa_amd_index_doc_match_list
    assert lst(fake, p, pat, 2, gc_, fl, 2, gq, 1, p, p, -1, c) == EINVAL                        # negative capacity
    assert lst(fake, p, pat, 2, gc_, fl, 2, gq, 1, None, p, 4, c) == EINVAL                      # NULL list_off, total_out
    assert lst(fake, p, pat, 2, gc_, fl, 2, gq, 1, p, p, 4, None) == EINVAL
    assert lst(fake, p, pat, 2, gc_, fl, 2, gq, 1, p, None, 4, c) == EINVAL                      # NULL docs with capacity > 0
    assert tot.value == -5 and np.all(buf == 0x77777777)
    assert sa.last_doc_match_stats() == before                        # a rejected call leaves the statistics alone
    L.sa_amd_last_doc_match_stats(None)


def test_budget_switch():
    try:
        assert sa.doc_match_set_budget(1 << 20) == sa.DOC_MATCH_BUDGET_DEFAULT
        assert sa.doc_match_set_budget(0) == 1 << 20
        assert sa.doc_match_set_budget(1 << 50) == BUDGET_MIN
        assert sa.doc_match_set_budget(-1) == BUDGET_MAX
        assert sa.doc_match_set_budget(-7) == sa.DOC_MATCH_BUDGET_DEFAULT
        assert sa.doc_match_set_budget(4097) == sa.DOC_MATCH_BUDGET_DEFAULT and sa.doc_match_set_budget(-1) == 4097
    finally:
        sa.doc_match_set_budget(-1)
