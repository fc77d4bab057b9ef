"""GPU suite for scoring a token text under the infinity-gram model on the token index:
sa_amd_tok_index_infgram_score compared bit for bit with score_by_bisection of tests/test_tok_score_abi.py (pinned there to the
definition and to brute force), on an index built on the device and on one created from the reference array; canaries around
every output, every output NULL in turn, the statistics against the models of tests/test_score_abi.py (the gallop, the long
decision and the work bounds do not depend on the symbol type), the index's own infgram and search on explicit prompts, and the
byte instantiation on a text over symbols below 256.

Sizes: texts of 2 500 .. 6 000 tokens, queries up to 1 500 positions (six tiles of 256); group caps 1, 63 and 65 make the staged
window start 2 modulo 4, and odd text positions make T + p do so."""
import functools
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_ngram_abi import ceil_log2
from test_score_abi import NAMES, doc_starts, effective_group_cap, gallop_bound, gallop_model, predicted_long_positions, search_steps_bound
from test_tok_score_abi import EXAMPLE_QUERY, TokenText, score_by_bisection
from test_tokens_abi import EXAMPLE_SA, EXAMPLE_TEXT, as_tokens, be_image, even_entries_halved, fibonacci_tokens

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
PAD = 32
CAPS = (0, 1, 63, 64, 65, 4096)
GROUP_CHUNK = 16                                                      # tokens a group of 8 lanes compares a round, charged whole
WAVE_CHUNK = 64                                                       # the long path's wave compare
KINDS = ("zipf", "period2", "one_token", "fibonacci", "zeros_ffff", "crossed")


# ---------------------------------------------------------------- the texts and their indexes ----

@functools.lru_cache(maxsize=None)
def text(kind):
    """-> TokenText (tokens, reference suffix array): computed once, shared, never changed"""
    rng = np.random.default_rng(len(kind))
    if kind == "zipf":
        t = corpus.token_corpus(6000, 50000, 11)
    elif kind == "period2":
        t = np.resize(np.array([0x0100, 0x0001]), 3001)
    elif kind == "one_token":
        t = np.full(2500, 0x0100)
    elif kind == "fibonacci":
        t = np.array(fibonacci_tokens(3000, 1, 256))
    elif kind == "zeros_ffff":
        t = np.where(rng.random(3000) < 0.5, 0x0000, 0xFFFF)
    elif kind == "crossed":                                            # the first differing BYTE of two tokens misleads
        t = np.array([0x0102, 0x0201, 0x0101, 0x0202])[rng.integers(0, 4, 4000)]
    elif kind == "below_256":
        t = rng.integers(0, 6, 5000)
        t[rng.choice(5000, 40, replace=False)] = 200
    else:
        raise KeyError(kind)
    from conftest import Oracle
    tok = as_tokens(t)
    tok.setflags(write=False)
    T = TokenText(tok, even_entries_halved(Oracle().sais(be_image(tok))))
    return T


class World:
    """per text the two indexes (built on the device, created from the reference array); opened on first use, closed together"""

    def __init__(self):
        self.open = {}

    def indexes(self, kind):
        if kind not in self.open:
            T = text(kind)
            self.open[kind] = (("built", sa.TokenIndex(T.tok)), ("given", sa.TokenIndex(T.tok, np.array(T.arr, dtype=np.uint32))))
        return self.open[kind]

    def close(self):
        for pair in self.open.values():
            for _, ix in pair:
                ix.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    try:
        yield w
    finally:
        w.close()


def absent_token(T):
    have = set(int(x) for x in np.unique(T.tok))
    return next(c for c in (60000, 0x1234, 7) if c not in have)


def substituted(q, rate, seed, absent):
    rng = np.random.default_rng(seed)
    q = np.array(q, dtype=np.uint16)
    q[rng.choice(q.size, max(1, int(q.size * rate)), replace=False)] = absent
    return q


def composite_query(T):
    """the text from its start (contexts reach back to position 0), a slice with substitutions, absent tokens, 0xFFFF and 0x0000,
    the text's last tokens with one more behind them (a context that is the text's tail) -> (query, document offsets)"""
    t, absent = T.tok, absent_token(T)
    parts = [t[:700], substituted(t[1001:1001 + 513], 0.01, 5, absent), [absent] * 3 + list(t[5:9]),
             [0xFFFF, 0x0000, 0xFFFF, 0xFFFF, 0x0000] + list(t[:3]), list(t[-200:]) + [absent]]
    q = as_tokens(np.concatenate([np.asarray(p, dtype=np.uint16) for p in parts]))
    off = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    return q, off


# ---------------------------------------------------------------- the calls ----

def raw_score(ix, q, q_off, min_count, max_len, null=()):
    """sa_amd_tok_index_infgram_score on numpy buffers with canaries around every output; the outputs named in `null` are passed
    as NULL -> dict of what was written (None for a NULL output) and the statistics"""
    q = as_tokens(q)
    m = q.size
    bufs = {k: np.full(m + 2 * PAD, 0xA5 if k == "at_end" else FILL32, dtype=np.uint8 if k == "at_end" else np.uint32) for k in NAMES}
    fill = {k: v[0].copy() for k, v in bufs.items()}
    off = None if q_off is None else np.ascontiguousarray(q_off, dtype=np.int64)
    args = [None if k in null else bufs[k][PAD:].ctypes.data for k in NAMES]
    rc = sa.lib().sa_amd_tok_index_infgram_score(ix._h, q.ctypes.data if m else None, m, None if off is None else off.ctypes.data,
                                                 0 if off is None else off.size - 1, min_count, max_len, *args)
    assert rc == 0, rc
    out = {"stats": sa.last_tok_score_stats()}
    for k, buf in bufs.items():                                       # nothing before, nothing behind, nothing at all through NULL
        w = 0 if k in null else m
        assert np.all(buf[:PAD] == fill[k]) and np.all(buf[PAD + w:] == fill[k]), k
        out[k] = None if k in null else buf[PAD:PAD + m].astype(np.int64)
    return out


_DEFS = {}


def definition(T, q, q_off, min_count, max_len):
    """score_by_bisection, computed once per case and shared"""
    q = as_tokens(q)
    key = (id(T), q.tobytes(), None if q_off is None else tuple(int(x) for x in q_off), min_count, max_len)
    if key not in _DEFS:
        d = score_by_bisection(T, q, q_off, min_count, max_len)
        for v in d.values():
            v.setflags(write=False)
        _DEFS[key] = d
    return _DEFS[key]


def check_stats(st, d, n, m, q_off, min_count, max_len, cap):
    """the statistics against the models: exact where the model is, inside the bound where it is a bound"""
    ge = effective_group_cap(cap, max_len)
    start = doc_starts(m, q_off)
    group, long_, longs, probes = [], [], 0, 0
    for j in range(m):
        s = int(d["s"][j])
        _, g, l, is_long = gallop_model(lambda x: x <= s, min(j - int(start[j]), max_len), ge)
        group += g
        long_ += l
        longs += is_long
        probes += gallop_bound(s)                                     # 2 ceil(log2(S + 2)) + 2
    assert longs == predicted_long_positions(m, q_off, d["s"], max_len, cap)
    if all(min(j - int(start[j]), max_len) <= ge for j in range(m)):
        assert longs == 0
    want = {"positions": m, "documents": 1 if q_off is None else len(q_off) - 1, "group_cap": ge, "long_positions": longs,
            "zero_positions": int(np.count_nonzero(d["nhi"] == d["nlo"])), "group_searches": len(group), "long_searches": len(long_),
            "readbacks": (1 + (longs > 0)) if m else 0}
    assert {k: st[k] for k in want} == want, (st, want)
    assert st["range_searches"] == len(group) + len(long_) <= probes
    steps = search_steps_bound(n)
    bound = steps * (sum(GROUP_CHUNK * -(-s // GROUP_CHUNK) for s in group) + sum(WAVE_CHUNK * -(-s // WAVE_CHUNK) for s in long_))
    assert 0 <= st["compared_tokens"] <= bound, (st, bound)
    assert 0 <= st["next_lookups"] <= 2 * m * (ceil_log2(n + 2) + 1)
    return longs


def check(ix, T, q, q_off=None, min_count=1, max_len=sa.SCORE_MAX_CONTEXT, cap=-1, where=None):
    """one call against the definition and its statistics against the models"""
    d = definition(T, q, q_off, min_count, max_len)
    prev = sa.score_set_group_cap(cap)
    try:
        got = raw_score(ix, q, q_off, min_count, max_len)
    finally:
        sa.score_set_group_cap(prev)
    for k in NAMES:
        bad = np.flatnonzero(got[k] != d[k])[:4]
        assert bad.size == 0, (k, where, cap, min_count, max_len, [(int(j), int(got[k][j]), int(d[k][j])) for j in bad])
    longs = check_stats(got["stats"], d, T.n, len(q), q_off, min_count, max_len, cap)
    return got, longs


# ---------------------------------------------------------------- the tests ----

def test_empty_text_empty_query_and_the_header_example():
    E = TokenText(np.zeros(0, dtype=np.uint16), [0])                   # n = 0: one slot, every context but the empty one is absent
    for ix in (sa.TokenIndex([]), sa.TokenIndex([], np.array([0], dtype=np.uint32))):
        got, _ = check(ix, E, [1, 2, 1, 0xFFFF])
        assert not got["s"].any() and got["hi"].tolist() == [1] * 4 and got["nlo"].tolist() == got["nhi"].tolist() == [1] * 4
        assert raw_score(ix, [], None, 1, 4)["stats"]["positions"] == 0
        ix.close()
    T = TokenText(as_tokens(EXAMPLE_TEXT), EXAMPLE_SA)
    for ix in (sa.TokenIndex(EXAMPLE_TEXT), sa.TokenIndex(EXAMPLE_TEXT, np.array(EXAMPLE_SA, dtype=np.uint32))):
        for cap in CAPS:
            got, _ = check(ix, T, EXAMPLE_QUERY, None, 1, 4, cap)
            assert [got[k].tolist() for k in NAMES] == [[0, 0, 1, 2], [0, 0, 4, 4], [6, 6, 6, 6], [1, 1, 0, 0], [4, 4, 4, 5], [4, 6, 6, 6]]
            assert not check(ix, T, EXAMPLE_QUERY, None, 3, 4, cap)[0]["s"].any()
        got = raw_score(ix, [], None, 1, 4)                            # m = 0 succeeds and writes nothing
        assert got["stats"]["positions"] == 0 and got["stats"]["readbacks"] == 0 and got["s"].size == 0
        assert raw_score(ix, [], [0, 0, 0], 1, 4)["stats"]["documents"] == 2
        r = ix.infgram_score(EXAMPLE_QUERY, 1, 4)                      # the Python surface and its result object
        assert isinstance(r, sa.ScoreResult) and r.s.tolist() == [0, 0, 1, 2] and r.at_end.dtype == np.uint8 and r.nhi.dtype == np.uint32
        cnt, den = r.counts()
        assert cnt.tolist() == [0, 2, 2, 1] and den.tolist() == [5, 5, 2, 2]
        assert np.isneginf(r.log2_prob()[0]) and r.log2_prob()[3] == pytest.approx(-1.0) and r.doc_bits([0, 2, 4])[1].tolist() == [1, 0]
        assert ix.infgram_score(np.array(EXAMPLE_QUERY, dtype=np.uint16), max_len=4, doc_offsets=[0, 2, 2, 4]).s.tolist() == [0, 0, 0, 1]
        ix.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_text_on_both_indexes(world, kind):
    """the composite query as one document and as five, under the default cap, every position long (0) and none (4 096)"""
    T = text(kind)
    q, off = composite_query(T)
    for name, ix in world.indexes(kind):
        for q_off in (None, off):
            for cap in (-1, 0, 4096):
                got, longs = check(ix, T, q, q_off, cap=cap, where=(kind, name))
                assert (cap == 4096) == (longs == 0)
    assert int(got["s"][:700].max()) == 699                            # the text from its start: every context reaches back to 0
    absent_at = int(off[2])
    assert got["nhi"][absent_at] == got["nlo"][absent_at] and got["s"][absent_at + 1] == 0
    if kind == "zipf":                                                 # the text's last 200 tokens occur only there: denominator 0
        j = len(q) - 1
        assert (got["s"][j], got["at_end"][j], got["hi"][j] - got["lo"][j]) == (200, 1, 1) and got["nhi"][j] == got["nlo"][j]
        r = world.indexes(kind)[0][1].infgram_score(q, doc_offsets=off)
        assert r.counts()[1][j] == 0 and np.isneginf(r.log2_prob()[j])


@pytest.mark.parametrize("kind", ["one_token", "period2", "crossed"])
def test_the_text_itself(world, kind):
    """query = T: the contexts reach max_len, or the whole prefix where it is 4 096"""
    T = text(kind)
    ix = world.indexes(kind)[0][1]
    q = T.tok[:1500]
    for max_len, cap in ((4096, -1), (4096, 4096), (64, -1), (65, 65), (63, 0)):
        got, longs = check(ix, T, q, None, 1, max_len, cap, where=kind)
        assert got["s"].tolist() == [min(j, max_len) for j in range(len(q))]
        assert (longs > 0) == (effective_group_cap(cap, max_len) < max_len)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 513])
def test_query_lengths_around_the_tile(world, m):
    """slices of the text from an odd position: the contexts reach back over the tile's start, into the staged halo"""
    T = text("zipf")
    q = substituted(T.tok[2001:2001 + m], 0.02, m, absent_token(T))
    for name, ix in world.indexes("zipf"):
        for cap in (-1, 1, 4096):
            got, _ = check(ix, T, q, cap=cap, where=name)
    assert m < 255 or (int(got["s"].max()) > 20 and (m < 257 or int(got["s"][256:].max()) > 2))


@pytest.mark.parametrize("max_len", [1, 2, 63, 64, 65, 4096])
def test_context_caps_under_every_group_cap(world, max_len):
    """group caps 1, 63 and 65 put the staged window at 2 modulo 4; the answers are those of every other cap"""
    T = text("crossed")
    ix = world.indexes("crossed")[1][1]
    q = np.concatenate((substituted(T.tok[1501:1501 + 300], 0.01, max_len, 0x0301), T.tok[777:777 + 330]))
    first = None
    for cap in CAPS:
        got, _ = check(ix, T, q, [0, 300, len(q)], 1, max_len, cap)
        first = first or got
        assert all(np.array_equal(got[k], first[k]) for k in NAMES)
    assert int(got["s"].max()) == min(max_len, 329)


def test_min_counts(world):
    for kind in ("zipf", "fibonacci"):
        T = text(kind)
        q, off = composite_query(T)
        for min_count in (1, 2, 3, T.n + 2):
            got, _ = check(world.indexes(kind)[0][1], T, q[600:1400], None, min_count, 4096, 63)
            assert np.all((got["s"] == 0) | (got["hi"] - got["lo"] >= min_count))
        assert not got["s"].any() and np.all(got["hi"] - got["lo"] == T.n + 1) and np.all(got["at_end"] == 1)    # n + 2: the unigram model


def test_document_starts_and_empty_documents(world):
    T = text("fibonacci")
    q = T.tok[301:301 + 513]
    m = len(q)
    tables = {"first of a tile": [0, 256, m], "last of a tile": [0, 255, 511, m], "mid tile": [0, 100, 300, 301, m],
              "empty documents": [0, 0, 0, 200, 200, 256, 256, 400, m, m, m], "every position": list(range(m + 1))}
    for name, ix in world.indexes("fibonacci"):
        for where, off in tables.items():
            for cap in (-1, 1, 4096):
                got, _ = check(ix, T, q, off, cap=cap, where=(name, where))
            start = doc_starts(m, off)
            assert np.all(got["s"] <= np.arange(m) - start) and np.all(got["s"][np.isin(np.arange(m), off)] == 0), where
    one, _ = check(ix, T, q, [0, m])                                   # ndocs = 1 is q_off = NULL
    none, _ = check(ix, T, q, None)
    assert all(np.array_equal(one[k], none[k]) for k in NAMES) and int(none["s"][-1]) == m - 1


def test_every_output_may_be_null(world):
    T = text("zipf")
    ix = world.indexes("zipf")[0][1]
    q, off = composite_query(T)
    q = q[650:950]
    d = definition(T, q, None, 1, 4096)
    for name in NAMES:
        got = raw_score(ix, q, None, 1, 4096, null=(name,))
        assert got[name] is None and all(np.array_equal(got[k], d[k]) for k in NAMES if k != name), name
    got = raw_score(ix, q, None, 1, 4096, null=NAMES)                  # everything NULL: only the statistics
    assert got["stats"]["positions"] == len(q) and got["stats"]["zero_positions"] == int(np.count_nonzero(d["nhi"] == d["nlo"]))


def test_invalid_arguments_write_nothing(world):
    ix = world.indexes("crossed")[0][1]
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    before = sa.last_tok_score_stats()
    for off, ndocs, min_count, max_len, m in (([0, 4], 1, 0, 8, 4), ([0, 4], 1, 1, 0, 4), ([0, 4], 1, 1, 4097, 4), ([0, 3], 1, 1, 8, 4),
                                              ([1, 4], 1, 1, 8, 4), ([0, 3, 2, 4], 3, 1, 8, 4), ([0, 4], -1, 1, 8, 4), ([0, 4], 1, 1, 8, -1)):
        a = np.array(off, dtype=np.int64)
        assert L.sa_amd_tok_index_infgram_score(ix._h, p, m, a.ctypes.data, ndocs, min_count, max_len, p, p, p, p, p, p) == -1, off
    assert L.sa_amd_tok_index_infgram_score(ix._h, p + 1, 4, None, 0, 1, 8, p, p, p, p, p, p) == -1        # a query at an odd address
    assert np.all(buf == 0x77777777) and sa.last_tok_score_stats() == before
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score([1, 2, 3], max_len=0)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score([1, 2, 3], doc_offsets=[0, 2])


@pytest.mark.parametrize("kind", ["zipf", "crossed", "zeros_ffff"])
def test_agreement_with_infgram_and_search(world, kind):
    """64 sampled positions: (S, LO, HI, AT_END) is TokenIndex.infgram of the prompt Q[start .. j), and [NLO, NHI) is
    TokenIndex.search of context + token where it occurs"""
    T = text(kind)
    q, off = composite_query(T)
    start = doc_starts(len(q), off)
    rng = np.random.default_rng(64)
    fixed = [int(off[2]), int(off[2]) + 3, int(off[3]), len(q) - 1]      # absent tokens (no continuation) and tokens behind them
    rest = np.setdiff1d(np.arange(len(q)), fixed)
    sample = np.sort(np.concatenate((fixed, rng.choice(rest, 64 - len(fixed), replace=False)))).astype(np.int64)
    for name, ix in world.indexes(kind):
        for min_count, max_len in ((1, 4096), (2, 65)):
            got, _ = check(ix, T, q, off, min_count, max_len, where=name)
            prompts = [q[int(start[j]):j] for j in sample]
            s, lo, hi, ae = ix.infgram(prompts, min_count, max_len)[:4]
            for k, v in zip(NAMES[:4], (s, lo, hi, ae)):
                assert np.array_equal(got[k][sample], v.astype(np.int64)), ("infgram", k, name)
            full = [q[j - int(got["s"][j]):j + 1] for j in sample]
            lo, hi = ix.search(full)
            occurs = hi > lo
            assert np.array_equal(occurs, got["nhi"][sample] > got["nlo"][sample]) and occurs.any() and not occurs.all()
            assert np.array_equal(lo[occurs], got["nlo"][sample][occurs]) and np.array_equal(hi[occurs], got["nhi"][sample][occurs])
            assert np.array_equal(lo[~occurs], got["nlo"][sample][~occurs])         # the insertion point


def test_agreement_with_the_byte_instantiation():
    """symbols below 256: a byte index without tables and a token index give identical six arrays and equal counters under the
    group caps 0, default and 4 096 (the compared-symbol counters are charged per round of different width: not compared)"""
    T = text("below_256")
    b = T.tok.astype(np.uint8)
    q = np.concatenate((b[:400], substituted(b[2001:2701], 0.01, 3, 201).astype(np.uint8), b[-50:], [201], b[40:300])).astype(np.uint8)
    off = [0, 400, 1100, 1151, len(q)]
    bytes_ix = sa.DeviceIndex(b)                                       # (no buckets(), no enable_lcp(): the plain route)
    tok_ix = sa.TokenIndex(T.tok)
    try:
        assert np.array_equal(bytes_ix.suffix_array(), tok_ix.sa())
        for cap in (0, -1, 4096):
            prev = sa.score_set_group_cap(cap)
            try:
                for min_count, max_len in ((1, 4096), (2, 70)):
                    rb = bytes_ix.infgram_score(q, min_count, max_len, off)
                    sb = sa.last_score_stats()
                    rt = tok_ix.infgram_score(q.astype(np.uint16), min_count, max_len, off)
                    st = sa.last_tok_score_stats()
                    for k, x, y in zip(NAMES, rb, rt):
                        assert x.dtype == y.dtype and np.array_equal(x, y), (k, cap)
                    for k in ("positions", "documents", "group_cap", "readbacks", "group_searches", "long_searches", "next_lookups",
                              "long_positions", "zero_positions"):
                        assert sb[k] == st[k], (k, cap, sb[k], st[k])
                    assert sb["compared_bytes"] > 0 and st["compared_tokens"] > 0
                d = definition(T, q.astype(np.uint16), off, 2, 70)
                assert all(np.array_equal(d[k], np.asarray(v, dtype=np.int64)) for k, v in zip(NAMES, rt))
            finally:
                sa.score_set_group_cap(prev)
        assert int(tok_ix.infgram_score(q.astype(np.uint16), 1, 70, off).s.max()) == 70
    finally:
        bytes_ix.close()
        tok_ix.close()


def test_an_array_that_is_no_suffix_array_is_survived():
    """a rotation of the right entries behind SA[0] = n (every entry in range, so the index accepts it): the answers are
    unspecified; the calls return, LO <= HI <= n + 1 and nothing is written outside the outputs"""
    T = text("zipf")
    arr = np.array(T.arr, dtype=np.uint32)
    wrong = np.concatenate((arr[:1], np.roll(arr[1:], 1237))).astype(np.uint32)
    assert wrong[0] == T.n and not np.array_equal(wrong, arr)
    ix = sa.TokenIndex(T.tok, wrong)
    q, off = composite_query(T)
    try:
        for cap in CAPS:
            prev = sa.score_set_group_cap(cap)
            try:
                for min_count, max_len in ((1, 4096), (2, 7)):
                    got = raw_score(ix, q, off, min_count, max_len)
                    assert np.all(got["lo"] <= got["hi"]) and np.all(got["hi"] <= T.n + 1)
            finally:
                sa.score_set_group_cap(prev)
    finally:
        ix.close()


def test_two_threads_with_different_group_caps(world):
    T = text("fibonacci")
    ix = world.indexes("fibonacci")[0][1]
    queries = [substituted(T.tok[101:1301], 0.01, 20 + j, 7) for j in range(2)]
    defs = [definition(T, q, None, 1, 4096) for q in queries]
    caps = (0, 4096)
    errors = []

    def work(j):
        try:
            sa.score_set_group_cap(caps[j])                            # (the switch is the calling thread's)
            for _ in range(3):
                got = raw_score(ix, queries[j], None, 1, 4096)
                assert all(np.array_equal(got[k], defs[j][k]) for k in NAMES)
                assert got["stats"]["group_cap"] == caps[j] and got["stats"]["positions"] == len(queries[j])
                assert (got["stats"]["long_positions"] > 0) == (caps[j] == 0) and (got["stats"]["group_searches"] == 0) == (caps[j] == 0)
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.score_set_group_cap(-1) == sa.SCORE_GROUP_CAP_DEFAULT    # the workers' switches were their own: this thread's is untouched


def test_the_other_features_statistics_are_left_untouched(world):
    T = text("below_256")
    b = T.tok.astype(np.uint8)
    bytes_ix = sa.DeviceIndex(b)
    tok_ix = sa.TokenIndex(T.tok)
    try:
        bytes_ix.infgram_score(b[:300], 1, 64)
        bytes_ix.infgram([b[50:90].tobytes(), b"q"], 2)
        tok_ix.infgram([T.tok[50:90], [9]], 2)
        readers = (sa.last_score_stats, sa.last_tok_stats, sa.last_ngram_stats, sa.last_stats)
        before = [f() for f in readers]
        tok_ix.infgram_score(T.tok[:2000], 1, 4096)
        assert [f() for f in readers] == before
        st = sa.last_tok_score_stats()
        assert st["positions"] == 2000 and st["long_positions"] > 0 and st["readbacks"] == 2
        bytes_ix.infgram_score(b[:300], 1, 64)                         # and the byte route leaves the token route's block alone
        assert sa.last_tok_score_stats() == st and sa.last_score_stats()["positions"] == 300
    finally:
        bytes_ix.close()
        tok_ix.close()
