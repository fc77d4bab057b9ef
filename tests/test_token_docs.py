"""GPU suite for document collections over the token indexes (include/sa_amd_tokdocs.h), both widths: the
header's example, the eight calls against the definitions of tests/test_token_docs_abi.py on the text families of
tests/test_tokens_abi.py, the separator pass at the sizes where its kernels change what they do, replacement and failure, the
capacities and canaries of every output, and the calls beside a caller's busy non-blocking stream.

The 32-bit index holds the same texts under the monotone map id -> 256 id + 255 (so 0xffff becomes 2^24 - 1, the top id): the
order of the suffixes, and with it every answer, is the 16-bit text's, and one definition serves both widths."""
import ctypes

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import Not
import test_streams as streams
from test_grid_laps import cu_count
from test_grid_laps_abi import tok_compact_lap
from test_token_docs_abi import (DOC_NONE, EINVAL, ERANGE, EXAMPLE_OFF, EXAMPLE_TEXT, LIMIT, PREFIXES, answers_definition,
                                 doc_of_definition, match_definition, queries_of, separator_offsets, word)
from test_tokens_abi import BRUTE_MAX, SPAN, TILE, as_tokens, brute_suffix_array, families

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32)
CLS = {16: sa.TokenIndex, 32: sa.TokenIndex32}
N = 600                                 # tokens of the family texts: brute force is the reference (<= BRUTE_MAX), ranges of many units at chunk 64
CHUNK_MIN, BUDGET_MIN = 64, 4096
CANARY32 = 0xA5A5A5A5
PAD = 16
assert N <= BRUTE_MAX


def widen(tokens, width):
    """the 16-bit tokens as the index of `width` holds them"""
    t = np.asarray(tokens, dtype=np.uint32).reshape(-1)
    return as_tokens(t) if width == 16 else (t * 256 + 255).astype(np.uint32)


def widen_queries(queries, width):
    def pat(p):
        return widen(p, width)

    def clause(c):
        if isinstance(c, Not):
            return Not(clause(c.clause))
        return pat(c) if sa._is_token_pattern(c) else [pat(p) for p in c]
    return [[clause(c) for c in q] for q in queries]


def device_answers(ix, width, pats, queries, pos):
    """the answers of the seven calls that read a collection, through the wrapper"""
    wp = [widen(p, width) for p in pats]
    occ, df = ix.doc_search(wp)
    mdf, cdf = ix.doc_match(widen_queries(queries, width), clause_df=True)
    return {"off": ix.doc_offsets().tolist(), "doc_of": ix.doc_of(pos).tolist(), "occ": occ.tolist(), "df": df.tolist(),
            "lists": [l.tolist() for l in ix.doc_list(wp)], "mdf": mdf.tolist(), "cdf": cdf.tolist(),
            "mlists": [l.tolist() for l in ix.doc_match_list(widen_queries(queries, width))]}


def defined_answers(t, arr, off, pats, queries, pos):
    occ, df, lists = answers_definition(t, off, arr, pats)
    mdf, cdf, mlists = match_definition(t, off, arr, queries)
    return {"off": [int(x) for x in off], "doc_of": doc_of_definition(off, len(t), pos).tolist(), "occ": occ.tolist(), "df": df.tolist(),
            "lists": [l.tolist() for l in lists], "mdf": mdf.tolist(), "cdf": cdf.tolist(), "mlists": [l.tolist() for l in mlists]}


def first_difference(got, want):
    for k in want:
        if got[k] != want[k]:
            return k
    return None


# ---------------------------------------------------------------- the header's example ----

@pytest.mark.parametrize("width", WIDTHS)
def test_header_example_on_the_device(width):
    ix = CLS[width](widen(EXAMPLE_TEXT, width))
    try:
        assert ix.ndocs == 0
        assert ix.set_documents(EXAMPLE_OFF) == 4 and ix.ndocs == 4
        assert ix.doc_offsets().tolist() == EXAMPLE_OFF
        assert ix.doc_of([0, 3, 4, 6, 7, 10, 11, DOC_NONE]).tolist() == [0, 0, 2, 2, 3, 3, DOC_NONE, DOC_NONE]
        w = lambda s: widen(word(s), width)                           # noqa: E731
        occ, df = ix.doc_search([w("a"), w("bra"), []])
        assert occ.tolist() == [5, 2, 12] and df.tolist() == [3, 2, 3]
        assert [l.tolist() for l in ix.doc_list([w("a"), w("bra")])] == [[3, 0, 2], [3, 0]]
        queries = [[w("a"), w("bra")], [w("a"), Not(w("bra"))], [Not(w("a"))], [[w("c"), w("bra")]], [w("ac")], [w("a"), w("c"), w("bra")], []]
        mdf, cdf = ix.doc_match(queries, clause_df=True)
        assert mdf.tolist() == [2, 1, 1, 3, 1, 0, 4] and cdf.tolist() == [3, 2, 3, 2, 1, 3, 1, 3, 1, 2]
        assert [l.tolist() for l in ix.doc_match_list(queries)] == [[0, 3], [2], [1], [0, 2, 3], [0], [], [0, 1, 2, 3]]
        r = int(widen(word("r"), width)[0])                           # "abr|acadabr|a"
        assert ix.set_documents(separator=r) == 3 and ix.doc_offsets().tolist() == [0, 3, 10, 11]
        assert ix.doc_search([w("a"), w("ra"), w("r")])[1].tolist() == [3, 2, 2]         # every r ends a document and belongs to it
        with pytest.raises(sa.SuffixArrayError):                      # offsets are integers: nothing is truncated on the way in
            ix.set_documents([0, 2.7, 11])
        assert ix.ndocs == 3
        one = np.array([0, 11], dtype=np.uint32)                      # set through the raw call: ndocs and doc_offsets are the library's
        assert getattr(sa.lib(), PREFIXES[width] + "set_documents")(ix._h, one.ctypes.data, 1) == 0
        assert ix.ndocs == 1 and ix.doc_offsets().tolist() == [0, 11]
        with pytest.raises(TypeError):
            ix.set_documents()
        with pytest.raises(TypeError):
            ix.set_documents(EXAMPLE_OFF, separator=r)
    finally:
        ix.close()


# ---------------------------------------------------------------- against the definitions ----

_FAMILY = {}


def family(name):
    """the family text of N tokens as a list of ints with its brute-force array; computed once, never changed"""
    if not _FAMILY:
        for k, v in families(N).items():
            t = [int(x) for x in v]
            _FAMILY[k] = (t, brute_suffix_array(t).tolist())
    return _FAMILY[name]


def collections(n, rng):
    cuts = np.sort(rng.integers(0, n + 1, 17))
    return {"one_document": [0, n],
            "every_token": list(range(n + 1)),
            "empty_documents": [0, 0, 0, n // 3, n // 3, n // 3, 2 * n // 3, n, n, n],
            "random_cuts": [0] + cuts.tolist() + [n]}


def patterns_for(t, off, rng):
    """the empty pattern, absent ones, ones that straddle a boundary, the most frequent token (in every document of the periodic
    families), substrings of several lengths and the whole text"""
    n = len(t)
    vals, counts = np.unique(np.array(t), return_counts=True)
    pats = [[], [int(vals[np.argmax(counts)])], [1, 2, 3], [0xFFFE], list(t), list(t[1:]) + [7]]
    inner = [c for c in off if 1 < c < n - 1]
    for c in inner[:3] + inner[-2:]:
        pats += [t[c - 1:c + 1], t[c - 2:c + 2]]
    for k in (1, 2, 3, 5, 64, 65):
        a = int(rng.integers(0, n - k))
        pats += [t[a:a + k], t[a:a + k - 1] + [(t[a + k - 1] + 1) & 0xFFFF]]
    return pats


@pytest.mark.parametrize("name", sorted(families(0)))
@pytest.mark.parametrize("width", WIDTHS)
def test_the_calls_against_the_definitions(width, name):
    t, arr = family(name)
    rng = np.random.default_rng(41)
    ix = CLS[width](widen(t, width))
    pos = np.concatenate((rng.integers(0, N, 200), [0, N - 1, N, N + 1, DOC_NONE])).astype(np.uint32)
    try:
        for cname, off in collections(N, rng).items():
            pats = patterns_for(t, off, rng)
            queries = queries_of(pats, rng) + [[Not(p) if k % 3 == 0 else p for k, p in enumerate(pats) if len(p)]] * 3
            want = defined_answers(t, arr, off, pats, queries, pos)
            assert ix.set_documents(off) == len(off) - 1
            for chunk, budget in ((CHUNK_MIN, BUDGET_MIN), (-1, -1)):
                prev_chunk, prev_budget = sa.docs_set_chunk(chunk), sa.doc_match_set_budget(budget)
                try:
                    got = device_answers(ix, width, pats, queries, pos)
                    assert first_difference(got, want) is None, (name, cname, chunk, first_difference(got, want))
                    if name == "one_token":                            # a pattern that occurs in every document that has a token
                        assert pats[1] == [0x0100] and got["df"][1] == int(np.count_nonzero(np.diff(off))), cname
                    ms = sa.last_doc_match_stats()
                    assert ms["readbacks"] == 1 and ms["listed"] == 1 and ms["df_sum"] == sum(want["mdf"])
                    if chunk == CHUNK_MIN and cname == "every_token":
                        assert ms["slabs"] > 1 and ms["budget"] == BUDGET_MIN          # the queries were split
                    ix.doc_search([widen(p, width) for p in pats])
                    ds = sa.last_docs_stats()
                    assert ds["readbacks"] == 1 and ds["occ_sum"] == sum(want["occ"]) and ds["df_sum"] == sum(want["df"])
                    units = sum(-(-o // (CHUNK_MIN if chunk == CHUNK_MIN else 4096)) for o in want["occ"])
                    assert ds["units"] == units and want["occ"][0] == N + 1 > 9 * CHUNK_MIN       # the empty pattern's range: one unit, and ten
                finally:
                    sa.docs_set_chunk(prev_chunk)
                    sa.doc_match_set_budget(prev_budget)
    finally:
        ix.close()


# ---------------------------------------------------------------- the separator pass ----

SEP = 0xFFFF                            # 16-bit: the top id; the 32-bit index holds it as 2^24 - 1
BIG = TILE * SPAN


def _text_with(n, at, seed):
    """n tokens over five ids, the separator exactly at the positions `at`"""
    t = np.random.default_rng(seed).integers(1, 6, n).astype(np.int64)
    if len(at):
        t[np.asarray(at, dtype=np.int64)] = SEP
    return t


def _sprinkled(n, seed, extra=()):
    rng = np.random.default_rng(seed)
    at = np.flatnonzero(rng.random(n) < 0.02).tolist() + [a for a in extra if 0 <= a < n]
    return _text_with(n, sorted(set(at)), seed + 1)


def separator_shapes():
    s = {"empty": _text_with(0, [], 1),
         "one_token_the_separator": _text_with(1, [0], 2),
         "one_token_another": _text_with(1, [], 3),
         "no_separator": _text_with(100, [], 4),
         "all_separators": _text_with(100, range(100), 5),
         "all_separators_past_a_tile": _text_with(TILE + 1, range(TILE + 1), 6),
         "first_and_last": _text_with(50, [0, 49], 7),
         "runs": _text_with(64, [10, 11, 12, 40, 41, 62, 63], 8),
         "at_the_tile_edges": _text_with(BIG + 5, [TILE - 1, TILE, BIG - 1, BIG], 9),
         "thirteen": _sprinkled(13, 10, [12]),                        # no multiple of the tokens of a 16-byte load
         "a_tile_and_three": _sprinkled(TILE + 3, 11, [TILE + 2])}
    for n in (TILE - 1, TILE, TILE + 1, BIG - 1, BIG, BIG + 1):
        s[f"n_{n}"] = _sprinkled(n, 12 + n, [n - 1] if n % 2 else [n - 2])
    return s


SHAPES = separator_shapes()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("width", WIDTHS)
def test_documents_by_separator(width, shape):
    t16 = SHAPES[shape]
    n = t16.size
    sep = int(widen([SEP], width)[0])
    assert sep == LIMIT[width] - 1                                    # 0xffff on the 16-bit index, 2^24 - 1 on the 32-bit one
    want = separator_offsets(t16, SEP)
    ix = CLS[width](widen(t16, width))
    rng = np.random.default_rng(5)
    t = t16.tolist()
    pats = [[], [SEP], [1], [2, 3], [SEP, SEP], [1, SEP, 2], [9]] + [t[a:a + k] for k in (1, 2, 4) for a in rng.integers(0, max(n - k, 1), 3).tolist()]
    queries = queries_of([p for p in pats if len(p)], rng)
    pos = np.concatenate((rng.integers(0, n + 2, 64), [0, n, DOC_NONE])).astype(np.uint32)
    try:
        ndocs = ix.set_documents(separator=sep)
        assert ndocs == want.size - 1 == int(np.count_nonzero(t16 == SEP)) + int(n == 0 or t16[-1] != SEP)
        assert np.array_equal(ix.doc_offsets(), want), shape
        by_separator = device_answers(ix, width, pats, queries, pos)
        assert ix.set_documents(np.array([0, n], dtype=np.uint32)) == 1 and ix.doc_offsets().tolist() == [0, n]      # (replaced in between)
        assert ix.set_documents(want) == ndocs
        by_offsets = device_answers(ix, width, pats, queries, pos)
        assert first_difference(by_separator, by_offsets) is None, (shape, first_difference(by_separator, by_offsets))
        assert by_offsets["doc_of"] == doc_of_definition(want, n, pos).tolist()
        assert by_offsets["occ"][1] == int(np.count_nonzero(t16 == SEP)) and by_offsets["df"][1] == by_offsets["occ"][1]      # one separator a document
    finally:
        ix.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_documents_by_separator_past_one_lap_of_the_grid(width):
    """A text just past one lap of tok_stream_grid (cu_count() * 8 workgroups of TK_SPAN tiles) with a partial last tile:
    separators at seeded random positions and one in the last partial tile.  Only the offsets and a sample of doc_of are
    compared, and neither depends on the suffix array, so the index is created from the identity array (in range, entry 0 is
    n: what create checks) instead of sorting sixteen million suffixes."""
    lap = tok_compact_lap(cu_count())
    n = lap + 3 * TILE + 5
    assert n > lap and n % TILE and (n - lap) // TILE >= 3
    rng = np.random.default_rng(77)
    t16 = rng.integers(0, 4, n).astype(np.uint16)
    at = np.unique(np.concatenate((rng.integers(0, n, 5000), [0, lap - 1, lap, lap + TILE, n - 3])))
    t16[at] = SEP
    sep = int(widen([SEP], width)[0])
    want = separator_offsets(t16, SEP)
    arr = np.concatenate(([n], np.arange(n))).astype(np.uint32)
    ix = CLS[width](widen(t16, width), arr)
    try:
        assert ix.set_documents(separator=sep) == want.size - 1
        got = ix.doc_offsets()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        pos = np.concatenate((rng.integers(0, n, 4000), at[-40:], at[-40:] + 1, [0, lap - 1, lap, n - 1, n])).astype(np.uint32)
        assert np.array_equal(ix.doc_of(pos), doc_of_definition(want, n, pos))
    finally:
        ix.close()


# ---------------------------------------------------------------- replacement and failure ----

def _raw(width):
    L = sa.lib()
    return {op: getattr(L, PREFIXES[width] + op) for op in sa.TOKEN_DOC_OPS}


@pytest.mark.parametrize("width", WIDTHS)
def test_replacement_failure_and_a_query_before_any_collection(width):
    t, arr = family("below_256")
    fn = _raw(width)
    ix = CLS[width](widen(t, width))
    rng = np.random.default_rng(3)
    pats = patterns_for(t, [0, N], rng)[:12]
    queries = queries_of(pats, rng)[:10]
    pos = np.arange(0, N + 2, 7, dtype=np.uint32)
    data, off, cnt = ix._batch([widen(p, width) for p in pats])
    buf = np.full(64, CANARY32, dtype=np.uint32)
    tot = ctypes.c_int64(-5)
    p, c = buf.ctypes.data, ctypes.byref(tot)
    one_off = np.array([0, 1], dtype=np.int32)
    one = one_off.ctypes.data
    try:
        # before any collection: every call that reads one is SA_AMD_EINVAL, nothing written
        assert fn["doc_offsets"](ix._h, p, 4, c) == EINVAL and fn["doc_of"](ix._h, pos.ctypes.data, 4, p) == EINVAL
        assert fn["doc_search"](ix._h, data.ctypes.data, off.ctypes.data, cnt, p, p) == EINVAL
        assert fn["doc_list"](ix._h, data.ctypes.data, off.ctypes.data, cnt, p, p, 4, c) == EINVAL
        assert fn["doc_match"](ix._h, data.ctypes.data, off.ctypes.data, 1, one, None, 1, one, 1, p, p) == EINVAL
        assert fn["doc_match_list"](ix._h, data.ctypes.data, off.ctypes.data, 1, one, None, 1, one, 1, p, p, 4, c) == EINVAL
        assert tot.value == -5 and np.all(buf == CANARY32)
        first, second = collections(N, rng)["random_cuts"], collections(N, rng)["empty_documents"]
        assert ix.set_documents(first) == len(first) - 1
        want_first = defined_answers(t, arr, first, pats, queries, pos)
        assert first_difference(device_answers(ix, width, pats, queries, pos), want_first) is None
        # rejected calls leave it answering: offsets that do not end at n, that decrease, a separator that is no token
        for bad in ([0, 5, N - 1], [0, 9, 5, N], [1, N]):
            b = np.array(bad, dtype=np.uint32)
            assert fn["set_documents"](ix._h, b.ctypes.data, b.size - 1) == EINVAL, bad
        assert fn["set_documents_by_separator"](ix._h, LIMIT[width], c) == ERANGE and tot.value == -5
        assert ix.ndocs == len(first) - 1
        assert first_difference(device_answers(ix, width, pats, queries, pos), want_first) is None
        # a second collection replaces the first, and the separator's replaces that
        assert ix.set_documents(second) == len(second) - 1
        assert first_difference(device_answers(ix, width, pats, queries, pos), defined_answers(t, arr, second, pats, queries, pos)) is None
        sep = int(widen([t[5]], width)[0])
        third = separator_offsets(np.array(t), t[5])
        assert ix.set_documents(separator=sep) == third.size - 1
        assert first_difference(device_answers(ix, width, pats, queries, pos), defined_answers(t, arr, third, pats, queries, pos)) is None
        if width == 32:                                               # a pattern id that is no token: SA_AMD_ERANGE, nothing written
            ids = np.array([1, 1 << 24], dtype=np.uint32)
            two = np.array([0, 2], dtype=np.int64)
            assert fn["doc_search"](ix._h, ids.ctypes.data, two.ctypes.data, 1, p, p) == ERANGE
            assert fn["doc_match_list"](ix._h, ids.ctypes.data, two.ctypes.data, 1, one, None, 1, one, 1, p, p, 4, c) == ERANGE
            assert tot.value == -5 and np.all(buf == CANARY32)
    finally:
        ix.close()


# ---------------------------------------------------------------- outputs ----

def _canaried(count, dtype=np.uint32):
    return np.full(int(count) + 2 * PAD, 0xA5, dtype=np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype)


def _holds(a, used):
    raw, w = a.view(np.uint8), a.itemsize
    return bool(np.all(raw[:PAD * w] == 0xA5) and np.all(raw[(PAD + used) * w:] == 0xA5))


def _ptr(a):
    return a[PAD:].ctypes.data


@pytest.mark.parametrize("width", WIDTHS)
def test_capacities_canaries_null_outputs_and_empty_batches(width):
    t, arr = family("period_2")
    fn = _raw(width)
    ix = CLS[width](widen(t, width))
    rng = np.random.default_rng(9)
    offs = collections(N, rng)["random_cuts"]
    pats = patterns_for(t, offs, rng)[:10]
    queries = queries_of(pats, rng)
    want = defined_answers(t, arr, offs, pats, queries, np.zeros(0, dtype=np.uint32))
    data, off, cnt = ix._batch([widen(p, width) for p in pats])
    qd, qoff, npat, coff, cfl, ncl, qo, nq = ix._queries(widen_queries(queries, width))
    pargs = (data.ctypes.data, off.ctypes.data, cnt)
    qargs = (qd.ctypes.data, qoff.ctypes.data, npat, coff.ctypes.data, cfl.ctypes.data, ncl, qo.ctypes.data, nq)
    try:
        ix.set_documents(offs)
        M = len(offs)
        for capacity in (0, 1, M - 1, M, M + 7):                      # doc_offsets: below, at and above ndocs + 1
            out, nd = _canaried(M + 7), _canaried(1, np.int64)
            assert fn["doc_offsets"](ix._h, _ptr(out) if capacity else None, capacity, _ptr(nd)) == 0
            wr = min(capacity, M)
            assert _holds(out, wr) and _holds(nd, 1) and nd[PAD] == M - 1 and out[PAD:PAD + wr].tolist() == offs[:wr]
        flat = [d for l in want["lists"] for d in l]
        loffs = np.concatenate(([0], np.cumsum([len(l) for l in want["lists"]]))).tolist()
        for capacity in (len(flat) + 9, len(flat), len(flat) - 1, 1, 0):
            lo, docs, tot = _canaried(cnt + 1, np.int64), _canaried(len(flat) + 9), _canaried(1, np.int64)
            assert fn["doc_list"](ix._h, *pargs, _ptr(lo), _ptr(docs) if capacity else None, capacity, _ptr(tot)) == 0
            wr = min(capacity, len(flat))
            assert _holds(lo, cnt + 1) and _holds(docs, wr) and _holds(tot, 1) and tot[PAD] == len(flat)
            assert lo[PAD:PAD + cnt + 1].tolist() == loffs and docs[PAD:PAD + wr].tolist() == flat[:wr]
            assert sa.last_docs_stats()["readbacks"] == 1 and sa.last_docs_stats()["listed"] == 1
        mflat = [d for l in want["mlists"] for d in l]
        mloffs = np.concatenate(([0], np.cumsum([len(l) for l in want["mlists"]]))).tolist()
        for capacity in (len(mflat) + 9, len(mflat), len(mflat) - 1, 1, 0):
            lo, docs, tot = _canaried(nq + 1, np.int64), _canaried(len(mflat) + 9), _canaried(1, np.int64)
            assert fn["doc_match_list"](ix._h, *qargs, _ptr(lo), _ptr(docs) if capacity else None, capacity, _ptr(tot)) == 0
            wr = min(capacity, len(mflat))
            assert _holds(lo, nq + 1) and _holds(docs, wr) and _holds(tot, 1) and tot[PAD] == len(mflat)
            assert lo[PAD:PAD + nq + 1].tolist() == mloffs and docs[PAD:PAD + wr].tolist() == mflat[:wr]
            assert sa.last_doc_match_stats()["readbacks"] == 1
        occ, df = _canaried(cnt), _canaried(cnt)
        assert fn["doc_search"](ix._h, *pargs, _ptr(occ), _ptr(df)) == 0 and _holds(occ, cnt) and _holds(df, cnt)
        assert occ[PAD:PAD + cnt].tolist() == want["occ"] and df[PAD:PAD + cnt].tolist() == want["df"]
        assert sa.last_docs_stats()["readbacks"] == 1 and sa.last_docs_stats()["listed"] == 0
        for a, b in ((None, _ptr(df)), (_ptr(occ), None), (None, None)):                    # NULL optional outputs
            assert fn["doc_search"](ix._h, *pargs, a, b) == 0
        mdf, cdf = _canaried(nq), _canaried(ncl)
        assert fn["doc_match"](ix._h, *qargs, _ptr(mdf), _ptr(cdf)) == 0 and _holds(mdf, nq) and _holds(cdf, ncl)
        assert mdf[PAD:PAD + nq].tolist() == want["mdf"] and cdf[PAD:PAD + ncl].tolist() == want["cdf"]
        for a, b in ((None, _ptr(cdf)), (_ptr(mdf), None), (None, None)):
            assert fn["doc_match"](ix._h, *qargs, a, b) == 0
        nd = _canaried(1, np.int64)
        assert fn["set_documents_by_separator"](ix._h, int(widen([t[0]], width)[0]), None) == 0        # NULL ndocs_out
        assert fn["doc_offsets"](ix._h, None, 0, _ptr(nd)) == 0 and nd[PAD] == separator_offsets(np.array(t), t[0]).size - 1
        # empty batches: nothing but list_off[0] and the total is written
        lo, docs, tot = _canaried(1, np.int64), _canaried(4), _canaried(1, np.int64)
        assert fn["doc_search"](ix._h, data.ctypes.data, off.ctypes.data, 0, _ptr(occ), _ptr(df)) == 0 and _holds(occ, cnt)
        assert fn["doc_list"](ix._h, data.ctypes.data, off.ctypes.data, 0, _ptr(lo), _ptr(docs), 4, _ptr(tot)) == 0
        assert lo[PAD] == 0 and tot[PAD] == 0 and _holds(lo, 1) and _holds(tot, 1) and _holds(docs, 0)
        zero32, zero64 = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
        zero, z64 = zero32.ctypes.data, zero64.ctypes.data
        lo, tot = _canaried(1, np.int64), _canaried(1, np.int64)
        assert fn["doc_match_list"](ix._h, data.ctypes.data, z64, 0, zero, None, 0, zero, 0, _ptr(lo), _ptr(docs), 4, _ptr(tot)) == 0
        assert lo[PAD] == 0 and tot[PAD] == 0 and _holds(lo, 1) and _holds(tot, 1) and _holds(docs, 0)
        assert fn["doc_match"](ix._h, data.ctypes.data, z64, 0, zero, None, 0, zero, 0, _ptr(mdf), _ptr(cdf)) == 0
        assert fn["doc_of"](ix._h, None, 0, None) == 0
    finally:
        ix.close()


# ---------------------------------------------------------------- beside a caller's busy stream ----

@pytest.mark.parametrize("width", WIDTHS)
def test_calls_neither_need_nor_disturb_a_busy_non_blocking_stream(width):
    """the eight calls while a caller's non-blocking stream is busy with unrelated copies (the delay chain of
    tests/test_streams.py): they answer correctly without that stream having drained, and its own work comes out untouched"""
    t, arr = family("zipf_50000")
    rng = np.random.default_rng(13)
    offs = collections(N, rng)["random_cuts"]
    pats = patterns_for(t, offs, rng)[:12]
    queries = queries_of(pats, rng)[:12]
    pos = np.arange(0, N + 2, 5, dtype=np.uint32)
    want = defined_answers(t, arr, offs, pats, queries, pos)
    third = separator_offsets(np.array(t), t[5])
    want_sep = defined_answers(t, arr, third, pats, queries, pos)
    ix = CLS[width](widen(t, width))
    env = streams.Env()
    hip = env.hip
    S = env.stream()
    try:
        pattern = np.arange(streams.SCRATCH // 8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        assert hip.hipMemcpy(env.scratch[0], pattern.ctypes.data, streams.SCRATCH, streams.H2D) == 0
        assert hip.hipMemset(env.scratch[1], 0, streams.SCRATCH) == 0
        assert hip.hipDeviceSynchronize() == 0

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        ix.set_documents(offs)
        assert first_difference(device_answers(ix, width, pats, queries, pos), want) is None

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        ix.set_documents(separator=int(widen([t[5]], width)[0]))
        assert first_difference(device_answers(ix, width, pats, queries, pos), want_sep) is None

        assert hip.hipStreamSynchronize(S) == 0
        back = np.empty_like(pattern)
        for p in env.scratch:                                         # an even number of copies each: both buffers hold the pattern
            assert hip.hipMemcpy(back.ctypes.data, p, streams.SCRATCH, streams.D2H) == 0
            assert np.array_equal(back, pattern)
    finally:
        hip.hipStreamSynchronize(S)
        hip.hipStreamDestroy(S)
        env.close()
        ix.close()
