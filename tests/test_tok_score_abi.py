"""CPU suite for scoring a token text under the infinity-gram model on the token index: the definition of
include/suffix_array_amd.h (S, LO, HI, AT_END, NLO, NHI per query position) restated over infgram_definition of
tests/test_tokens_abi.py and checked slot by slot against brute force on the raw tokens, the identities that tie it to the
other token queries, the header's example, the exports and the Python surface, the argument checks that answer without a
device, and a model of the group compare of kernels/match.hpp at two tokens a word.  tests/test_tok_score.py imports the
definition from here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import TokScoreStats, last_tok_score_stats      # (the feature's surface: without it nothing below is collected)
from conftest import ROOT
from test_score_abi import NAMES, doc_starts
from test_tokens_abi import (EXAMPLE_SA, EXAMPLE_TEXT, brute_suffix_array, infgram_definition, next_tokens_definition, range_definition,
                             small_cases)

EXPORTS = ("sa_amd_tok_index_infgram_score", "sa_amd_last_tok_score_stats")
STATS_FIELDS = ("positions", "documents", "group_searches", "long_searches", "next_lookups", "compared_tokens", "long_positions",
                "zero_positions", "group_cap", "readbacks")
EXAMPLE_QUERY = [7, 256, 1, 256]
GROUP = 8                                                             # SCORE_G: lanes that serve one position
WORD_TOKENS = 2                                                       # tokens a lane compares a round: one 32-bit word


# ---------------------------------------------------------------- the definition ----

def score_definition(t, arr, q, q_off, min_count, max_len):
    """-> dict of int64 arrays s / lo / hi / at_end / nlo / nhi over the positions of the query.  t, q: lists of ints, arr: the
    token suffix array.  infgram_definition of the prompt Q[start .. j) gives the first four; its listing gives
    NLO = LO + AT_END + sum(next[t'] for t' < Q[j]) and NHI = NLO + next[Q[j]]"""
    assert max_len >= 1
    m = len(q)
    out = {k: np.zeros(m, dtype=np.int64) for k in NAMES}
    start = doc_starts(m, q_off)
    for j in range(m):
        s, lo, hi, ae, listing = infgram_definition(t, arr, q[int(start[j]):j], min_count, max_len)
        nlo = lo + ae + sum(c for v, c in listing if v < q[j])
        nhi = nlo + sum(c for v, c in listing if v == q[j])
        for k, v in zip(NAMES, (s, lo, hi, ae, nlo, nhi)):
            out[k][j] = v
    return out


def brute_score(t, q, q_off, min_count, max_len):
    """the same from the raw tokens alone, looking at every slot: occurrences counted by slicing, every length tried longest
    first, a slot number as the count of the suffixes (the empty one included) that sort below the string"""
    n, m = len(t), len(q)
    out = {k: np.zeros(m, dtype=np.int64) for k in NAMES}
    start = doc_starts(m, q_off)

    def occurrences(x):
        return sum(1 for i in range(n + 1) if t[i:i + len(x)] == x)

    def below(x):
        return sum(1 for i in range(n + 1) if t[i:i + len(x)] < x)
    for j in range(m):
        cap = min(j - int(start[j]), max_len)
        s = next((k for k in range(cap, 0, -1) if occurrences(q[j - k:j]) >= min_count), 0)
        ctx = q[j - s:j]
        full = ctx + [q[j]]
        row = (s, below(ctx), below(ctx) + occurrences(ctx), int(t[n - s:] == ctx), below(full), below(full) + occurrences(full))
        for k, v in zip(NAMES, row):
            out[k][j] = v
    return out


class TokenText:
    """a token text and its suffix array prepared for score_by_bisection: token slices compare as slices of the big-endian byte
    image (equal order, one memcmp)"""

    def __init__(self, tok, arr):
        self.tok = np.ascontiguousarray(tok, dtype=np.uint16)
        self.n = int(self.tok.size)
        self.be = self.tok.astype(">u2").tobytes()
        self.arr = [int(x) for x in arr]
        assert len(self.arr) == self.n + 1

    def range(self, pat_be):
        be, arr, p = self.be, self.arr, len(pat_be)
        lo, hi = 0, self.n + 1
        while lo < hi:
            m = (lo + hi) // 2
            if be[2 * arr[m]:2 * arr[m] + p] < pat_be:
                lo = m + 1
            else:
                hi = m
        lo2, hi2 = lo, self.n + 1
        while lo2 < hi2:
            m = (lo2 + hi2) // 2
            if be[2 * arr[m]:2 * arr[m] + p] == pat_be:
                lo2 = m + 1
            else:
                hi2 = m
        return lo, lo2


def score_by_bisection(T, q, q_off, min_count, max_len):
    """score_definition for the texts of thousands of tokens of the GPU suite: the count never grows with the context's length, so S
    is found by bisection; NLO / NHI are two lower bounds on the token behind the context, which is sorted inside the range.
    test_bisection_is_the_definition pins it to score_definition."""
    q = np.ascontiguousarray(q, dtype=np.uint16)
    qbe = q.astype(">u2").tobytes()
    m, n, arr, tok = int(q.size), T.n, T.arr, T.tok
    out = {k: np.zeros(m, dtype=np.int64) for k in NAMES}
    start = doc_starts(m, q_off)
    for j in range(m):
        good, bad, lo, hi = 0, min(j - int(start[j]), max_len) + 1, 0, n + 1
        while bad - good > 1:
            s = (good + bad) // 2
            r = T.range(qbe[2 * (j - s):2 * j])
            if r[1] - r[0] >= min_count:
                good, lo, hi = s, r[0], r[1]
            else:
                bad = s
        ae = int(hi > lo and arr[lo] + good == n)
        bounds = []
        for target in (int(q[j]), int(q[j]) + 1):
            a, b = lo + ae, hi
            while a < b:
                mid = (a + b) // 2
                at = arr[mid] + good
                if (int(tok[at]) if at < n else 65536) < target:
                    a = mid + 1
                else:
                    b = mid
            bounds.append(a)
        for k, v in zip(NAMES, (good, lo, hi, ae, bounds[0], bounds[1])):
            out[k][j] = v
    return out


def queries_of(t, rng):
    """(query, q_off) pairs: pieces of the text with one substituted token, 0x0000 and 0xFFFF, a token the text lacks, the text's
    last tokens at a document's end, empty documents at the front, in the middle and at the end"""
    n = len(t)
    have = set(t)
    absent = next(c for c in range(65535, -1, -1) if c not in have)
    parts = []
    for _ in range(3):
        if n:
            a = int(rng.integers(0, n))
            piece = list(t[a:a + int(rng.integers(1, 16))])
            parts.append(list(piece))
            piece[int(rng.integers(0, len(piece)))] ^= 0x0101
            parts.append(piece)
    parts += [[absent] + t[:3], [0xFFFF, 0x0000] + t[:2] + [0xFFFF], t[-7:] + [absent]]      # (the last context is the text's tail: at_end)
    q = [x for p in parts for x in p]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    holes = np.concatenate([[0, 0], off[:3], off[2:], [len(q)]]).astype(np.int64)
    return [(q, None), (q, off), (q, holes)]


# ---------------------------------------------------------------- the tests of the definition ----

def test_definition_against_brute_force_and_the_identities():
    rng = np.random.default_rng(24)
    seen = 0
    for name, tok in small_cases():
        if tok.size > 300:
            continue
        t = [int(x) for x in tok]
        n = len(t)
        arr = brute_suffix_array(t).tolist()
        for q, q_off in queries_of(t, rng):
            start = doc_starts(len(q), q_off)
            for min_count, max_len in ((1, 4096), (2, 4096), (1, 1), (3, 2), (n + 2, 7)):
                d = score_definition(t, arr, q, q_off, min_count, max_len)
                if n <= 70 or (min_count, max_len) == (1, 4096):     # (slot-by-slot brute force is cubic: every setting on the small texts)
                    b = brute_score(t, q, q_off, min_count, max_len)
                    for k in NAMES:
                        assert np.array_equal(d[k], b[k]), (name, k, min_count, max_len)
                assert np.all(d["s"] <= np.minimum(np.arange(len(q)) - start, max_len))
                assert np.all((d["lo"] + d["at_end"] <= d["nlo"]) & (d["nlo"] <= d["nhi"]) & (d["nhi"] <= d["hi"]))
                if min_count == n + 2:
                    assert not d["s"].any() and np.all(d["hi"] - d["lo"] == n + 1) and np.all(d["at_end"] == 1)
                for j in range(len(q)):
                    s = int(d["s"][j])
                    prompt = q[int(start[j]):j]
                    # (S, LO, HI, AT_END) is infgram of the prompt Q[start .. j)
                    assert infgram_definition(t, arr, prompt, min_count, max_len)[:4] == tuple(int(d[k][j]) for k in NAMES[:4])
                    # [NLO, NHI) is the range of context + token, or has zero width at the insertion point
                    lo, hi = range_definition(t, arr, q[j - s:j + 1])
                    if hi > lo:
                        assert (lo, hi) == (int(d["nlo"][j]), int(d["nhi"][j])), (name, j)
                    else:
                        assert d["nlo"][j] == d["nhi"][j] == lo, (name, j)
                        clo, chi, ae, _ = next_tokens_definition(t, arr, q[j - s:j])
                        assert clo + ae <= lo <= chi
                seen += 1
    assert seen >= 5 * 3 * 30


def test_bisection_is_the_definition():
    """the GPU suite's reference equals score_definition on every small family, every query and setting"""
    rng = np.random.default_rng(25)
    for name, tok in small_cases():
        if tok.size > 300:
            continue
        t = [int(x) for x in tok]
        arr = brute_suffix_array(t).tolist()
        T = TokenText(tok, arr)
        for q, q_off in queries_of(t, rng):
            for min_count, max_len in ((1, 4096), (2, 4096), (1, 1), (3, 2), (len(t) + 2, 7)):
                d = score_definition(t, arr, q, q_off, min_count, max_len)
                f = score_by_bisection(T, q, q_off, min_count, max_len)
                for k in NAMES:
                    assert np.array_equal(d[k], f[k]), (name, k, min_count, max_len)


def test_the_header_example():
    t, arr, q = EXAMPLE_TEXT, EXAMPLE_SA, EXAMPLE_QUERY
    assert brute_suffix_array(t).tolist() == arr
    d = score_definition(t, arr, q, None, 1, 4)
    b = brute_score(t, q, None, 1, 4)
    assert all(np.array_equal(d[k], b[k]) for k in NAMES)
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    assert "T = {256, 1, 256, 1, 2}, SA = {5, 3, 1, 4, 2, 0}, Q = {7, 256, 1, 256}, one document, min_count = 1, max_len = 4:" in header
    assert " *     j  token  S  [LO, HI)  AT_END  [NLO, NHI)\n" in header
    for j in range(len(q)):                                           # every line rebuilt from the definition
        s, lo, hi, ae, nlo, nhi = (int(d[k][j]) for k in NAMES)
        line = f" *     {j}  {q[j]:<5d}  {s}  " + f"[{lo}, {hi})".ljust(10) + f"{ae}       [{nlo}, {nhi})\n"
        assert line in header, line
    assert [int(x) for x in d["s"]] == [0, 0, 1, 2] and [int(x) for x in d["nlo"]] == [4, 4, 4, 5]     # (and the issue's table)
    assert [int(x) for x in d["nhi"]] == [4, 6, 6, 6] and [int(x) for x in d["lo"]] == [0, 0, 4, 4]
    d3 = score_definition(t, arr, q, None, 3, 4)
    assert not d3["s"].any() and range_definition(t, arr, [256]) == (4, 6)
    assert "With min_count = 3, positions 2 and 3 have S = 0: {256} occurs twice." in header


# ---------------------------------------------------------------- the surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    body = header[header.index("typedef struct sa_amd_tok_score_stats"):header.index("} sa_amd_tok_score_stats;")]
    declared = re.findall(r"^\s+int(64|32)_t\s+(\w+);", body, re.M)
    assert sa.TokScoreStats is TokScoreStats and sa.last_tok_score_stats is last_tok_score_stats
    assert [name for _, name in declared] == list(STATS_FIELDS) == [name for name, _ in sa.TokScoreStats._fields_]
    for (bits, name), (_, ctype) in zip(declared, sa.TokScoreStats._fields_):
        assert ctypes.sizeof(ctype) * 8 == int(bits), name
    assert ctypes.sizeof(sa.TokScoreStats) == ctypes.sizeof(sa.ScoreStats) == 8 * 8 + 2 * 4
    assert [(n.replace("tokens", "bytes"), c) for n, c in sa.TokScoreStats._fields_] == list(sa.ScoreStats._fields_)
    plain = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    decls = dict(re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", plain))
    for fn in EXPORTS:                                                # host pointers only: no device form, no stream
        assert fn in decls and "stream" not in decls[fn], fn
    assert not any(name.startswith("sa_amd_tok") and name.endswith("_device") for name in decls)
    params = [p.strip() for p in decls["sa_amd_tok_index_infgram_score"].split(",")]
    assert params == ["const sa_amd_tok_index *ix", "const uint16_t *Q", "int64_t m", "const int64_t *q_off", "int64_t ndocs", "int32_t min_count",
                      "int32_t max_len", "uint32_t *S", "uint32_t *LO", "uint32_t *HI", "uint8_t *AT_END", "uint32_t *NLO", "uint32_t *NHI"]
    assert "counts context TOKENS" in header                          # the group cap's comment says that it applies here
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        hpp = f.read()
    assert "Score infgram_score(const Tokens &query" in hpp and "using Score = DocumentIndex::Score;" in hpp


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(sa.TokenIndex.infgram_score) == params(sa.DeviceIndex.infgram_score) == ["self", "query", "min_count", "max_len", "doc_offsets"]
    sig = inspect.signature(sa.TokenIndex.infgram_score)
    assert [sig.parameters[k].default for k in ("min_count", "max_len", "doc_offsets")] == [1, sa.SCORE_MAX_CONTEXT, None]
    assert sig.return_annotation in (sa.ScoreResult, "ScoreResult")       # the existing result class (annotations may be strings)
    for name in ("TokScoreStats", "last_tok_score_stats"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert params(sa.last_tok_score_stats) == []
    assert set(sa.last_tok_score_stats()) == set(STATS_FIELDS) | {"range_searches"}


def test_python_rejects_bad_tokens_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sa, "lib", no_library)
    ix = object.__new__(sa.TokenIndex)
    for bad, err in (([1, 65536], ValueError), ([-1], ValueError), ([1.5], TypeError), (["a"], TypeError), (b"ab", TypeError), ("ab", TypeError),
                     (np.zeros(3, dtype=np.uint8), TypeError), (np.zeros(3, dtype=np.int32), TypeError),
                     (np.zeros((2, 2), dtype=np.uint16), TypeError), ([True], TypeError)):
        with pytest.raises(err):
            ix.infgram_score(bad)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score([1, 2], min_count=0)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score([1, 2], doc_offsets=[[0, 2]])


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    g = good.ctypes.data
    before = sa.last_tok_score_stats()

    def call(ix, q, m, off, ndocs, min_count, max_len):
        return L.sa_amd_tok_index_infgram_score(ix, q, m, off, ndocs, min_count, max_len, p, p, p, p, p, p)
    assert call(None, p, 4, g, 2, 1, 8) == -1                                                    # NULL index
    assert call(None, p, 0, None, 0, 1, 8) == -1                                                 #   also with m == 0
    assert call(fake, p, -1, None, 0, 1, 8) == -1                                                # negative m
    assert call(fake, None, 4, None, 0, 1, 8) == -1                                              # no query
    assert call(fake, p + 1, 4, None, 0, 1, 8) == -1                                             # a query that is not 2-byte aligned
    assert call(fake, p, 4, g, -1, 1, 8) == -1                                                   # negative ndocs
    for min_count in (0, -1, -2**31):
        assert call(fake, p, 4, g, 2, min_count, 8) == -1
    for max_len in (0, -1, 4097, 2**31 - 1):
        assert call(fake, p, 4, g, 2, 1, max_len) == -1
    for off in ([1, 2, 4], [0, 3, 2], [0, 2, 5], [0, 2, 3], [-1, 2, 4], [0, 5, 4]):           # malformed q_off
        a = np.array(off, dtype=np.int64)
        assert call(fake, p, 4, a.ctypes.data, 2, 1, 8) == -1, off
    assert np.all(buf == 0x77777777) and sa.last_tok_score_stats() == before
    L.sa_amd_last_tok_score_stats(None)


# ---------------------------------------------------------------- the group compare at two tokens a word ----

def word_at(tokens, i):
    """the little-endian 32-bit word a lane loads at token i: tokens i and i + 1 (0 behind the end)"""
    a = tokens[i] if i < len(tokens) else 0
    b = tokens[i + 1] if i + 1 < len(tokens) else 0
    return a | (b << 16)


def group_compare_model(text, pat, frm, limit, lanes=GROUP):
    """match_group_lcp<G, uint16_t> of kernels/match.hpp: lane gl compares the word at token offset off + 2 gl, the tail of the
    last word is masked in TOKENS, the first differing lane is found, then the first differing token of its word, and the order
    is that of the two 16-bit VALUES.  -> (lcp, less, tokens charged)"""
    charged = 0
    off = frm
    while off < limit:
        found = None
        for gl in range(lanes):
            o = off + WORD_TOKENS * gl
            if o >= limit:
                continue
            left = limit - o
            mask = 0xFFFFFFFF if left >= WORD_TOKENS else (1 << (16 * left)) - 1
            tw, qw = word_at(text, o), word_at(pat, o)
            d = (tw ^ qw) & mask
            if d and found is None:
                found = (gl, d, tw, qw)
        charged += WORD_TOKENS * lanes
        if found:
            gl, d, tw, qw = found
            si = ((d & -d).bit_length() - 1) >> 4
            return off + WORD_TOKENS * gl + si, ((tw >> (16 * si)) & 0xFFFF) < ((qw >> (16 * si)) & 0xFFFF), charged
        off += WORD_TOKENS * lanes
    return limit, False, charged


def byte_order_compare(tw, qw, d):
    """what the byte instantiation's rule would say on a token word: the first differing BYTE decides (wrong for tokens)"""
    bi = ((d & -d).bit_length() - 1) >> 3
    return ((tw >> (8 * bi)) & 255) < ((qw >> (8 * bi)) & 255)


def list_compare(text, pat, limit):
    lcp = next((i for i in range(limit) if text[i] != pat[i]), limit)
    return lcp, (lcp < limit and text[lcp] < pat[lcp])


def test_token_word_compare_model():
    pairs = [(0x0102, 0x0201), (0x0201, 0x0102),                      # the byte orders crossed: the low byte says the opposite
             (0x0100, 0x0200), (0x0200, 0x0100), (0x01FF, 0xFF01),    # differ only in the high byte / crossed at the extremes
             (0x0001, 0x0002), (0x0102, 0x0101),                      # differ only in the low byte
             (0x0000, 0xFFFF), (0xFFFF, 0x0000), (0x00FF, 0x0100)]
    for a, b in pairs:
        for at in (0, 1, 2, 15, 16, 17, 30):                          # both tokens of a word, the group's last word, the next round
            for limit in (at + 1, at + 2, at + 3, 40):
                base = [0x0101 * (i % 7 + 1) for i in range(limit)]
                text, pat = list(base), list(base)
                text[at], pat[at] = a, b
                # garbage behind the limit must not show: the tail of a word is masked in tokens
                text_x, pat_x = text + [0x1111, 0x2222], pat + [0x3333, 0x0001]
                for frm in sorted({0, min(at, 1), at - at % 2, at}):
                    got = group_compare_model(text_x, pat_x, frm, limit)
                    assert got[:2] == list_compare(text, pat, limit), (hex(a), hex(b), at, limit, frm)
                    assert got[2] % (WORD_TOKENS * GROUP) == 0 and got[2] >= WORD_TOKENS * GROUP
    # one token left in the last word: half a word is compared, the other half is not
    assert group_compare_model([5, 9], [5, 7], 0, 1) == (1, False, 16)
    assert group_compare_model([5, 9], [5, 7], 0, 2) == (1, False, 16)
    assert group_compare_model([5, 6], [5, 7], 0, 2) == (1, True, 16)
    assert group_compare_model(list(range(40)), list(range(40)), 3, 36) == (36, False, 3 * 16)
    # the negative check: the byte rule gives the wrong order exactly on the crossed pairs
    tw, qw = 0x0102, 0x0201
    assert byte_order_compare(tw, qw, tw ^ qw) is False and (tw < qw) is True
    assert group_compare_model([tw], [qw], 0, 1)[:2] == (0, True)
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "score.hpp")) as f:
        assert re.search(r"constexpr int SCORE_G = (\d+);", f.read()).group(1) == str(GROUP)
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "match.hpp")) as f:
        src = f.read()                                                # the one piece of the compare that is specialised on Sym
    assert "match_word_diff<Sym>(df, tf, qf, less)" in src and "constexpr int W = 4 / (int)sizeof(Sym);" in src
