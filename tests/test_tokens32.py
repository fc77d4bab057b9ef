"""GPU suite for the 32-bit token texts, ids below 2^24: sa_amd_saca_u32 against the CPU reference on every
text family at the sizes where the construction changes its path, SA_AMD_ERANGE for a text id of 2^24 with nothing written, the
token index (built on the device and created from the reference array) against the definitions of tests/test_tokens_abi.py and
tests/test_tok_score_abi.py -- search, next_tokens and infgram with the stream cap forced to 0, at its default and at 2^31 - 1,
infgram_score under group caps that force the long list --, agreement with the 16-bit index on texts that fit it, the routes on
work blocks that hold each fill pattern of tests/dirty_blocks.py, and two calls beside a caller's busy non-blocking stream.

Sizes.  Construction: n around one work-item of the image pass (16 tokens), 3 n + 1 around one compaction tile (n = 682, 683) and
one span of four tiles (2 730, 2 731; there 3 n also crosses the 8 192 bytes of the byte builder's small-text route), n around
4 096, and n = 70 001 (the general route, many tiles); brute force is the reference up to 2 000 tokens, the oracle on the 3-byte
image above (the CPU suite pins that the two agree).  Index: 7 200 tokens -- the empty context's range is above the default
stream cap of 1 024, a planted id above 65 535 has 600 distinct continuations, half of which differ from the other half only in
their top byte."""
import ctypes

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import TokenIndex32, corpus, saca_u32
import dirty_blocks
import test_streams as streams
from test_tok_score_abi import NAMES, score_definition
from test_tokens32_abi import (EXAMPLE_QUERY, EXAMPLE_SA, EXAMPLE_TEXT, EXPORTS, LIMIT, as_tokens32, be_image3, families32,
                               reference_suffix_array32)
from test_tokens_abi import BRUTE_MAX, families, infgram_definition, next_tokens_definition, range_definition

pytestmark = pytest.mark.gpu

CANARY32 = 0xA5A5A5A5
PAD = 16                                # canary words on either side of an output
BUILD_SIZES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 682, 683, 2730, 2731, 4095, 4096, 4097, 70001)
CAPS = (0, -1, 2**31 - 1)               # every non-empty range searched; the default; every range streamed
HOT = 0x012345                          # the planted id of the index text, above 65 535: 600 distinct continuations
ERANGE = -6


def _saca_u32_raw(t):
    """sa_amd_saca_u32 through the library with canary words around the output -> (rc, the whole buffer)"""
    buf = np.full(t.size + 1 + 2 * PAD, CANARY32, dtype=np.uint32)
    rc = sa.lib().sa_amd_saca_u32(t.ctypes.data if t.size else None, buf[PAD:].ctypes.data, t.size)
    return rc, buf


def _saca_u32_canaried(t):
    rc, buf = _saca_u32_raw(t)
    assert rc == 0, rc
    assert np.all(buf[:PAD] == CANARY32) and np.all(buf[PAD + t.size + 1:] == CANARY32)
    return buf[PAD:PAD + t.size + 1].copy()


@pytest.mark.parametrize("n", BUILD_SIZES)
def test_saca_u32_against_the_reference(oracle, n):
    for name, t in families32(n).items():
        got = _saca_u32_canaried(t)
        want = reference_suffix_array32(t, oracle)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, n, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert np.array_equal(saca_u32(t), want), (name, n)
    st = sa.last_tok_stats()
    assert n == 0 or (st["image_ms"] >= 0 and st["build_ms"] > 0 and st["compact_ms"] > 0)


def test_header_example_and_what_cannot_stand_in():
    """the text that the 16-bit form on truncated ids, and a little-endian image, order differently"""
    assert saca_u32(EXAMPLE_TEXT).tolist() == EXAMPLE_SA
    assert sa.saca_u16([x & 0xFFFF for x in EXAMPLE_TEXT]).tolist() != EXAMPLE_SA
    assert saca_u32(np.array([0x010000, 0x000001], dtype=np.uint32)).tolist() == [2, 1, 0]
    assert saca_u32(np.array([0x000100, 0x000001], dtype=np.uint32)).tolist() == [2, 1, 0]
    assert saca_u32([]).tolist() == [0]
    assert saca_u32([LIMIT - 1, 0, LIMIT - 1]).tolist() == [3, 1, 2, 0]


@pytest.mark.parametrize("n", [1, 37, 5003])
def test_a_text_id_of_2_to_the_24_is_erange_with_nothing_written(oracle, n):
    """the id first, last, and in the tail group of the image pass (the last, partial 16 tokens): SA_AMD_ERANGE from the device,
    the output and its canaries untouched; the index forms refuse the text with and without a supplied array"""
    base = corpus.token_corpus_u32(n, 200000, 5)
    arr = reference_suffix_array32(base, oracle)
    for at in sorted({0, n - 1, n - n % 16 if n % 16 else n - 16, n // 2} & set(range(n))):
        for bad_id in (LIMIT, 0xFFFFFFFF):
            t = base.copy()
            t[at] = bad_id
            rc, buf = _saca_u32_raw(t)
            assert rc == ERANGE and np.all(buf == CANARY32), (n, at, rc)
            for given in (None, arr):
                with pytest.raises(sa.SuffixArrayError) as e:
                    TokenIndex32(t, given)
                assert e.value.code == ERANGE, (n, at, given is None)
    assert np.array_equal(_saca_u32_canaried(base), arr)              # the largest id that is a token, and the text itself
    top = base.copy()
    top[n - 1] = LIMIT - 1
    assert np.array_equal(_saca_u32_canaried(top), reference_suffix_array32(top, oracle))


# ---------------------------------------------------------------- the index ----

class Model:
    """the index text, its reference array and the two indexes; shared by the tests below, never changed"""

    def __init__(self, oracle):
        planted = np.empty(1200, dtype=np.uint32)
        planted[0::2] = HOT
        planted[1::2] = 1000 + np.arange(600) % 300 + (np.arange(600) // 300) * 0x010000      # 300 pairs that differ only in the top byte
        body = corpus.token_corpus_u32(6000, 200000, 9)
        self.tok = as_tokens32(np.concatenate((body[:3000], planted, body[3000:])))
        self.tok.setflags(write=False)
        self.t = [int(x) for x in self.tok]
        self.n = len(self.t)
        assert self.n > BRUTE_MAX
        self.arr = reference_suffix_array32(self.tok, oracle)
        self.arr.setflags(write=False)
        self.lst = self.arr.tolist()
        self.built = TokenIndex32(self.tok)
        self.given = TokenIndex32(self.tok, self.arr)
        self.indexes = (("built", self.built), ("given", self.given))

    def close(self):
        self.built.close()
        self.given.close()


@pytest.fixture(scope="module")
def model(oracle):
    m = Model(oracle)
    try:
        yield m
    finally:
        m.close()


def _inside_token_patterns(m):
    """tokens read from the byte image at offsets that are no multiple of 3: they occur in the image, but a match there starts
    inside a token"""
    b = be_image3(m.tok)
    out = []
    for a in (1, 2, 100, 2000, 9002, 18001):
        assert a % 3
        for k in (1, 2, 3):
            raw = b[a:a + 3 * k]
            out.append([(int(raw[3 * i]) << 16) | (int(raw[3 * i + 1]) << 8) | int(raw[3 * i + 2]) for i in range(k)])
    return out


def _search_patterns(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(17)
    pats = [[], list(t), list(t) + [5], [HOT], [HOT, 1000], [HOT, 0x010000 + 1000], [HOT, 999], [LIMIT - 1, LIMIT - 1], [0], [HOT & 0xFFFF]]
    for k in (1, 2, 5, 63, 64, 65, 66, 128, 129):                     # around the 64 tokens of a wave step
        a = int(rng.integers(0, n - k))
        pats.append(t[a:a + k])
        pats.append(t[a:a + k - 1] + [(t[a + k - 1] + 1) % LIMIT])     # differs in its last token
        pats.append(t[a:a + k - 1] + [t[a + k - 1] ^ 0x010000])        #   ... only in that token's top byte
        pats.append(t[n - k:])                                        # a suffix of the text
    return pats + _inside_token_patterns(m)


def test_index_holds_the_reference_array(model):
    for name, ix in model.indexes:
        assert np.array_equal(ix.sa(), model.arr), name
    assert len(model.built) == model.n


def test_search_against_the_definition(model):
    pats = _search_patterns(model)
    want = [range_definition(model.t, model.lst, p) for p in pats]
    for name, ix in model.indexes:
        lo, hi = ix.search(pats)
        assert [(int(a), int(b)) for a, b in zip(lo, hi)] == want, name
        assert ix.count(pats).tolist() == [b - a for a, b in want]
        assert ix.contains(pats).tolist() == [b > a for a, b in want]
    inside = _inside_token_patterns(model)
    image = be_image3(model.tok).tobytes()
    empty = 0
    for p in inside:
        assert be_image3(p).tobytes() in image                        # the byte image holds it ...
        lo, hi = range_definition(model.t, model.lst, p)
        empty += lo == hi                                             # ... but no token position does
    assert empty >= len(inside) // 2
    lo, hi = model.built.search([])
    assert lo.size == 0 and hi.size == 0


def _contexts(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(23)
    ctx = [[], [HOT], [HOT, 1000], t[n - 2:], t[n - 1:], list(t), [9, 9, 9], [HOT, 999]]
    for k in (1, 1, 1, 2, 2, 3, 7, 64, 65):
        a = int(rng.integers(0, n - k))
        ctx.append(t[a:a + k])
    vals, cnts = np.unique(m.tok, return_counts=True)
    return ctx + [[int(vals[cnts.argmax()])]]                         # the most frequent token


def _prompts(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(29)
    out = [[], [7], [7, HOT], list(t[n - 5:]), [3, 3] + t[100:110], t[200:330]]
    for k in (2, 5, 20):
        a = int(rng.integers(0, n - k))
        out.append([(t[a] + 1) % LIMIT] + t[a + 1:a + k])              # the first token breaks the match: a shorter suffix
        out.append(t[a:a + k] + [(t[a + k - 1] + 7) % LIMIT])
    return out


def _listing(loff, toks, counts, q):
    return [(int(a), int(b)) for a, b in zip(toks[loff[q]:loff[q + 1]], counts[loff[q]:loff[q + 1]])]


@pytest.mark.parametrize("cap", CAPS)
def test_next_tokens_against_the_definition(model, cap):
    ctx = _contexts(model)
    want = [next_tokens_definition(model.t, model.lst, c) for c in ctx]
    assert max(len(w[3]) for w in want) > 256 and 600 <= len(want[1][3]) and want[1][1] - want[1][0] <= 1024
    hot = [v for v, _ in want[1][3]]
    assert sum((v ^ 0x010000) in hot for v in hot) == 600 and max(hot) > 65535       # continuations that differ only in the top byte
    assert want[3][2] == 1 and want[0][2] == 1                                      # at_end
    prev = sa.ngram_set_stream_cap(cap)
    try:
        for name, ix in model.indexes:
            lo, hi, ae, loff, toks, counts = ix.next_tokens(ctx)
            assert toks.dtype == np.uint32
            for q, (wlo, whi, wae, wl) in enumerate(want):
                assert (int(lo[q]), int(hi[q]), int(ae[q])) == (wlo, whi, wae), (name, q)
                assert _listing(loff, toks, counts, q) == wl, (name, q)
            st = sa.last_tok_stats()
            assert st["patterns"] == len(ctx) and st["entries"] == loff[-1] == sum(len(w[3]) for w in want)
            assert st["backoff"] == 0 and st["passes"] == 2 and st["readbacks"] == 1 and st["compared_tokens"] == -1
            assert st["stream_queries"] + st["search_queries"] + st["empty_queries"] == len(ctx)
            if cap == 0:
                assert st["stream_queries"] == 0 and st["search_queries"] > 0
            if cap == 2**31 - 1:
                assert st["search_queries"] == 0 and st["stream_slots"] == sum(w[1] - w[0] - w[2] for w in want)
            if cap == -1:
                assert st["stream_cap"] == sa.NGRAM_STREAM_CAP_DEFAULT and st["stream_queries"] > 0 and st["search_queries"] > 0
    finally:
        sa.ngram_set_stream_cap(prev)


@pytest.mark.parametrize("cap", CAPS)
def test_infgram_against_the_definition(model, cap):
    prompts = _prompts(model)
    prev = sa.ngram_set_stream_cap(cap)
    try:
        for min_count, max_len in ((1, 0), (2, 0), (3, 4), (model.n + 5, 0)):
            want = [infgram_definition(model.t, model.lst, p, min_count, max_len) for p in prompts]
            for name, ix in model.indexes:
                s, lo, hi, ae, loff, toks, counts = ix.infgram(prompts, min_count, max_len)
                for q, (ws, wlo, whi, wae, wl) in enumerate(want):
                    assert (int(s[q]), int(lo[q]), int(hi[q]), int(ae[q])) == (ws, wlo, whi, wae), (name, q, min_count, max_len)
                    assert _listing(loff, toks, counts, q) == wl, (name, q)
                st = sa.last_tok_stats()
                assert st["backoff"] == 1 and st["readbacks"] == 1 and st["compared_tokens"] >= 0
                bound = sum((min(len(p), max_len) if max_len > 0 else len(p)).bit_length() for p in prompts)
                assert st["range_searches"] <= bound                  # ceil(log2(cap + 1)) = bit_length(cap) searches a prompt
    finally:
        sa.ngram_set_stream_cap(prev)


def test_header_example_on_the_device():
    for arr in (None, np.array(EXAMPLE_SA, dtype=np.uint32)):
        ix = TokenIndex32(EXAMPLE_TEXT, arr)
        lo, hi, ae, loff, toks, counts = ix.next_tokens([[65536, 1], [1], [2], [], [9]])
        assert list(zip(lo.tolist(), hi.tolist()))[:4] == [(4, 5), (1, 3), (3, 4), (0, 6)] and lo[4] == hi[4]
        assert ae.tolist() == [0, 0, 1, 1, 0]
        assert [_listing(loff, toks, counts, q) for q in range(5)] == [[(2, 1)], [(2, 1), (65536, 1)], [], [(1, 2), (2, 1), (65536, 1), (65537, 1)], []]
        for (min_count, max_len), want in (((1, 0), (2, 4, 5)), ((2, 0), (1, 1, 3)), ((3, 0), (0, 0, 6))):
            s, lo, hi = ix.infgram([[7, 65536, 1]], min_count, max_len)[:3]
            assert (int(s[0]), int(lo[0]), int(hi[0])) == want
        r = ix.infgram_score(EXAMPLE_QUERY, 1, 4)
        d = score_definition(EXAMPLE_TEXT, EXAMPLE_SA, EXAMPLE_QUERY, None, 1, 4)
        for k, got in zip(NAMES, (r.s, r.lo, r.hi, r.at_end, r.nlo, r.nhi)):
            assert got.astype(np.int64).tolist() == d[k].tolist(), k
        ix.close()


def _raw_query(ix, pats, capacity, backoff, outputs=True):
    """the library call itself with canaried output buffers -> (rc, total, dict of the arrays)"""
    data, off, cnt = sa._token_batch32(pats)
    L = sa.lib()

    def buf(count, dtype):
        a = np.empty(count + 2 * PAD, dtype=dtype)
        a.view(np.uint8)[:] = 0xA5
        return a

    out = {"slen": buf(cnt, np.uint32), "lo": buf(cnt, np.uint32), "hi": buf(cnt, np.uint32), "ae": buf(cnt, np.uint8),
           "loff": buf(cnt + 1, np.int64), "toks": buf(max(capacity, 0), np.uint32), "counts": buf(max(capacity, 0), np.uint32)}
    ptr = {k: (v[PAD:].ctypes.data if outputs else None) for k, v in out.items()}
    total = ctypes.c_int64(-7)
    tp = ctypes.byref(total) if outputs else None
    if backoff:
        rc = L.sa_amd_tok32_index_infgram(ix._h, data.ctypes.data, off.ctypes.data, cnt, 1, 0, ptr["slen"], ptr["lo"], ptr["hi"], ptr["ae"],
                                          ptr["loff"], ptr["toks"], ptr["counts"], capacity, tp)
    else:
        rc = L.sa_amd_tok32_index_next_tokens(ix._h, data.ctypes.data, off.ctypes.data, cnt, ptr["lo"], ptr["hi"], ptr["ae"], ptr["loff"],
                                              ptr["toks"], ptr["counts"], capacity, tp)
    sizes = {"slen": cnt if backoff else 0, "lo": cnt, "hi": cnt, "ae": cnt, "loff": cnt + 1}
    return rc, int(total.value), out, sizes


def _canaries_hold(a, used):
    raw = a.view(np.uint8)
    w = a.itemsize
    return bool(np.all(raw[:PAD * w] == 0xA5) and np.all(raw[(PAD + used) * w:] == 0xA5))


@pytest.mark.parametrize("backoff", [False, True])
def test_capacity_canaries_null_outputs_and_empty_batch(model, backoff):
    ctx = _contexts(model)[:6]
    want = [infgram_definition(model.t, model.lst, c, 1, 0)[1:] if backoff else next_tokens_definition(model.t, model.lst, c) for c in ctx]
    flat = [e for w in want for e in w[3]]
    for cap in CAPS:
        prev = sa.ngram_set_stream_cap(cap)
        try:
            for capacity in (len(flat) + 9, len(flat), 700, 1, 0):        # above, exactly, inside the second listing, one, none
                rc, total, out, sizes = _raw_query(model.built, ctx, capacity, backoff)
                assert rc == 0 and total == len(flat), (cap, capacity)
                wr = min(capacity, len(flat))
                for k, used in list(sizes.items()) + [("toks", wr), ("counts", wr)]:
                    assert _canaries_hold(out[k], used), (k, cap, capacity)
                assert [(int(a), int(b)) for a, b in zip(out["toks"][PAD:PAD + wr], out["counts"][PAD:PAD + wr])] == flat[:wr]
                assert out["loff"][PAD:PAD + len(ctx) + 1].tolist() == np.concatenate(([0], np.cumsum([len(w[3]) for w in want]))).tolist()
                assert out["lo"][PAD:PAD + len(ctx)].tolist() == [w[0] for w in want]
                assert sa.last_tok_stats()["passes"] == (2 if wr else 1)
        finally:
            sa.ngram_set_stream_cap(prev)
    rc, total, out, sizes = _raw_query(model.built, ctx, 50, backoff, outputs=False)      # every output NULL
    assert rc == 0 and total == -7 and all(_canaries_hold(a, 0) for a in out.values())
    assert sa.last_tok_stats()["entries"] == len(flat)
    rc, total, out, sizes = _raw_query(model.built, [], 4, backoff)                       # count == 0
    assert rc == 0 and total == 0 and out["loff"][PAD] == 0 and _canaries_hold(out["loff"], 1)
    assert all(_canaries_hold(out[k], 0) for k in ("slen", "lo", "hi", "ae", "toks", "counts"))


def test_search_outputs_canaries_and_nulls(model):
    pats = _search_patterns(model)[:12]
    data, off, cnt = sa._token_batch32(pats)
    want = [range_definition(model.t, model.lst, p) for p in pats]
    has = np.full(cnt + 2 * PAD, 0xA5, dtype=np.uint8)
    lo, hi = np.full(cnt + 2 * PAD, CANARY32, dtype=np.uint32), np.full(cnt + 2 * PAD, CANARY32, dtype=np.uint32)
    L = sa.lib()
    assert L.sa_amd_tok32_index_search(model.given._h, data.ctypes.data, off.ctypes.data, cnt, has[PAD:].ctypes.data, lo[PAD:].ctypes.data,
                                       hi[PAD:].ctypes.data) == 0
    assert all(_canaries_hold(a, cnt) for a in (has, lo, hi))
    assert list(zip(lo[PAD:PAD + cnt].tolist(), hi[PAD:PAD + cnt].tolist())) == want
    assert has[PAD:PAD + cnt].tolist() == [int(b > a) for a, b in want]
    assert L.sa_amd_tok32_index_search(model.given._h, data.ctypes.data, off.ctypes.data, cnt, None, None, None) == 0
    assert L.sa_amd_tok32_index_search(model.given._h, data.ctypes.data, off.ctypes.data, 0, None, None, None) == 0
    data = data.copy()
    data[3] = LIMIT                                                   # a pattern id that is no token: refused on the host, nothing written
    assert L.sa_amd_tok32_index_search(model.given._h, data.ctypes.data, off.ctypes.data, cnt, has[PAD:].ctypes.data, lo[PAD:].ctypes.data,
                                       hi[PAD:].ctypes.data) == ERANGE
    assert list(zip(lo[PAD:PAD + cnt].tolist(), hi[PAD:PAD + cnt].tolist())) == want


def test_a_supplied_array_is_range_checked(model):
    bad = model.arr.copy()
    bad[model.n // 2] = model.n + 1                                   # an entry above n
    with pytest.raises(sa.SuffixArrayError) as e:
        TokenIndex32(model.tok, bad)
    assert e.value.code == ERANGE
    bad = model.arr.copy()
    bad[0], bad[1] = bad[1], bad[0]                                   # in range, but SA[0] != n
    with pytest.raises(sa.SuffixArrayError) as e:
        TokenIndex32(model.tok, bad)
    assert e.value.code == -1
    wrong = np.roll(model.arr[1:], 5)                                 # in range and wrong: unspecified answers, nothing out of range
    ix = TokenIndex32(model.tok, np.concatenate((model.arr[:1], wrong)).astype(np.uint32))
    for cap in CAPS:
        prev = sa.ngram_set_stream_cap(cap)
        try:
            lo, hi, ae, loff, toks, counts = ix.next_tokens(_contexts(model))
            assert loff[-1] == toks.size == counts.size and np.all(hi <= model.n + 1)
            ix.infgram(_prompts(model), 2, 0)
            ix.infgram_score(model.tok[:300], 1, 16)
        finally:
            sa.ngram_set_stream_cap(prev)
    ix.close()


# ---------------------------------------------------------------- scoring ----

SCORE_MAX_LEN = 40
SCORE_NAMES = NAMES


def _score_query(m):
    """the text from its start, a slice with substitutions (one only in a top byte), ids the text lacks, the largest id and 0, the
    text's last tokens with one more behind them -> (query, document offsets)"""
    t = m.t
    have = set(t)
    absent = next(c for c in range(LIMIT - 1, -1, -1) if c not in have)
    piece = list(t[3001:3001 + 90])
    piece[17] ^= 0x010000
    piece[50] = absent
    parts = [t[:70], piece, [absent] * 3 + t[5:9], [LIMIT - 1, 0, LIMIT - 1] + t[:3], [HOT, 1000, HOT, 0x010000 + 1000, HOT], t[-60:] + [absent]]
    q = as_tokens32([x for p in parts for x in p])
    off = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    return q, off


_SCORE_DEFS = {}


def _score_want(m, q, off, min_count, max_len):
    """score_definition, computed once per case and shared"""
    key = (None if off is None else tuple(int(x) for x in off), min_count, max_len)
    if key not in _SCORE_DEFS:
        d = score_definition(m.t, m.lst, [int(x) for x in q], off, min_count, max_len)
        for v in d.values():
            v.setflags(write=False)
        _SCORE_DEFS[key] = d
    return _SCORE_DEFS[key]


def _raw_score(ix, q, q_off, min_count, max_len, shift):
    """sa_amd_tok32_index_infgram_score on a query whose address is `shift` modulo 8, canaries around every output"""
    m = q.size
    room = np.zeros(m + 8, dtype=np.uint32)
    base = room.ctypes.data
    first = ((shift - base) % 8) // 4
    assert (base + 4 * first) % 8 == shift
    room[first:first + m] = q
    room[:first] = LIMIT + 5                                          # what lies around the query is no token and is never read as one
    room[first + m:] = LIMIT + 5
    bufs = {k: np.full(m + 2 * PAD, 0xA5 if k == "at_end" else CANARY32, dtype=np.uint8 if k == "at_end" else np.uint32) for k in SCORE_NAMES}
    off = None if q_off is None else np.ascontiguousarray(q_off, dtype=np.int64)
    rc = sa.lib().sa_amd_tok32_index_infgram_score(ix._h, base + 4 * first, m, None if off is None else off.ctypes.data,
                                                   0 if off is None else off.size - 1, min_count, max_len,
                                                   *[bufs[k][PAD:].ctypes.data for k in SCORE_NAMES])
    assert rc == 0, rc
    out = {}
    for k, buf in bufs.items():
        fill = 0xA5 if k == "at_end" else CANARY32
        assert np.all(buf[:PAD] == fill) and np.all(buf[PAD + m:] == fill), k
        out[k] = buf[PAD:PAD + m].astype(np.int64)
    return out, sa.last_tok_score_stats()


@pytest.mark.parametrize("cap", [0, 1, 5, -1])
def test_infgram_score_against_the_definition(model, cap):
    """with document offsets and without, at query addresses 0 and 4 modulo 8; group caps below max_len send every position whose
    context reaches the cap to the long list"""
    q, off = _score_query(model)
    prev = sa.score_set_group_cap(cap)
    try:
        for q_off, min_count, shift in ((off, 1, 0), (off, 1, 4), (None, 1, 4), (off, 2, 0)):
            d = _score_want(model, q, q_off, min_count, SCORE_MAX_LEN)
            for name, ix in model.indexes:
                got, st = _raw_score(ix, q, q_off, min_count, SCORE_MAX_LEN, shift)
                for k in SCORE_NAMES:
                    bad = np.flatnonzero(got[k] != d[k])[:4]
                    assert bad.size == 0, (k, name, cap, shift, [(int(j), int(got[k][j]), int(d[k][j])) for j in bad])
                ge = min(64 if cap < 0 else cap, SCORE_MAX_LEN)
                assert st["positions"] == q.size and st["group_cap"] == ge
                assert st["zero_positions"] == int(np.count_nonzero(d["nhi"] == d["nlo"]))
                # a position goes to the long list iff its document has more than ge tokens before it and ge of them are good
                at = np.arange(q.size)
                start = np.zeros(q.size, dtype=np.int64) if q_off is None else q_off[np.searchsorted(q_off, at, side="right") - 1]
                longs = int(np.count_nonzero((np.minimum(at - start, SCORE_MAX_LEN) > ge) & (d["s"] >= ge)))
                assert st["long_positions"] == longs and st["readbacks"] == 1 + (longs > 0) and (st["long_searches"] > 0) == (longs > 0)
                assert longs > 0 or ge == SCORE_MAX_LEN or min_count > 1, (cap, longs)      # (every cap below max_len does force the long list)
        assert int(_score_want(model, q, off, 1, SCORE_MAX_LEN)["s"].max()) > 5       # contexts longer than the small caps exist
    finally:
        sa.score_set_group_cap(prev)
    r = model.built.infgram_score(q, 1, SCORE_MAX_LEN, doc_offsets=off)
    d = _score_want(model, q, off, 1, SCORE_MAX_LEN)
    assert all(np.array_equal(np.asarray(g, dtype=np.int64), d[k]) for k, g in zip(SCORE_NAMES, (r.s, r.lo, r.hi, r.at_end, r.nlo, r.nhi)))
    assert model.built.infgram_score([]).s.size == 0


# ---------------------------------------------------------------- agreement across widths ----

def _answers(ix, tok, rng_seed):
    """every kind of query above on an index over `tok` (ids below 65 536, so both widths can hold it)"""
    t = [int(x) for x in tok]
    n = len(t)
    rng = np.random.default_rng(rng_seed)
    pats = [[], [0], [65535], list(t[:3]), list(t[max(n - 2, 0):])]
    for k in (1, 2, 3, 7, 64, 65, 129):
        if n > k:
            a = int(rng.integers(0, n - k))
            pats.append(t[a:a + k])
            pats.append(t[a:a + k - 1] + [(t[a + k - 1] + 1) & 0xFFFF])
    out = [ix.sa()]
    out += list(ix.search(pats)) + [ix.count(pats), ix.contains(pats)]
    out += list(ix.next_tokens(pats))
    for min_count, max_len in ((1, 0), (2, 0), (3, 4)):
        out += list(ix.infgram(pats, min_count, max_len))
    q = t[:200] + t[n // 2:n // 2 + 100] + [65535, 0] + t[max(n - 50, 0):]
    off = [0, min(200, n), len(q) - 52, len(q)] if n >= 200 else None
    for cap in (1, -1):
        prev = sa.score_set_group_cap(cap)
        try:
            r = ix.infgram_score(q, 1, 32, doc_offsets=off)
        finally:
            sa.score_set_group_cap(prev)
        out += [r.s, r.lo, r.hi, r.at_end, r.nlo, r.nhi]
    return [np.asarray(a).astype(np.int64) for a in out]


def _widths_agree(tok16, seed):
    narrow, wide = sa.TokenIndex(tok16), TokenIndex32(tok16.astype(np.uint32))
    try:
        a, b = _answers(narrow, tok16, seed), _answers(wide, tok16, seed)
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (i, x[:4], y[:4])
    finally:
        narrow.close()
        wide.close()
    assert np.array_equal(saca_u32(tok16.astype(np.uint32)), sa.saca_u16(tok16))


def test_both_widths_answer_alike_on_the_token_corpus():
    _widths_agree(corpus.token_corpus(70001, 50000, 3), 41)


@pytest.mark.parametrize("n", [5, 257, 700])
def test_both_widths_answer_alike_on_the_16_bit_families(n):
    for name, tok16 in families(n).items():
        _widths_agree(tok16, 43)


# ---------------------------------------------------------------- work blocks that hold arbitrary bytes ----

DIRTY_FNS = tuple(fn for fn in EXPORTS if fn != "sa_amd_max_tokens_u32")      # (a size query: arithmetic on the host)


def _dirty_route(d, model):
    """every device entry point of the 32-bit token forms once, through the diagnostic library -> the answers"""
    used = set()
    out = []
    for n in (5, 37, 683, 2731, 5003):
        for name, t in families32(n).items():
            if name in ("zipf_200000", "top_byte_only", "period_3"):
                out.append(saca_u32(t))
    used.add("sa_amd_saca_u32")
    for arr in (None, model.arr):
        ix = d._track(TokenIndex32(model.tok, arr))
        out.append(ix.sa())
        out += list(ix.search(_search_patterns(model)))
        out += list(ix.next_tokens(_contexts(model)))
        out += list(ix.infgram(_prompts(model), 2, 0))
        q, off = _score_query(model)
        r = ix.infgram_score(q, 1, SCORE_MAX_LEN, doc_offsets=off)
        out += [r.s, r.lo, r.hi, r.at_end, r.nlo, r.nhi]
        ix.close()
    used |= {"sa_amd_tok32_index_" + op for op in ("create", "destroy", "sa", "search", "next_tokens", "infgram", "infgram_score")}
    assert used == set(DIRTY_FNS)
    return [np.asarray(a).copy() for a in out]


@pytest.mark.parametrize("pattern", dirty_blocks.ORDER)
def test_routes_on_dirty_blocks(model, oracle, pattern):
    """no answer depends on the bytes a work block, a table's allocation or the slack behind the tokens held before the call: the
    slack behind a text of n tokens is read by the image pass (16-byte loads) and must raise no range flag whatever it holds.
    (The diagnostic library is entered and left inside the test: the other tests of this module use the product's indexes.)"""
    with dirty_blocks.diag_library() as diag:
        assert diag.fill(None) == dirty_blocks.FILL_OFF
        clean = _dirty_route(diag, model)
        assert np.array_equal(clean[0], reference_suffix_array32(families32(5)["period_3"], oracle))
        diag.fill(pattern)
        try:
            got = _dirty_route(diag, model)
        finally:
            was = diag.fill(None)
        assert was == dirty_blocks.PATTERNS[pattern]
    assert len(got) == len(clean)
    for i, (x, y) in enumerate(zip(got, clean)):
        assert np.array_equal(x, y), (pattern, i)


# ---------------------------------------------------------------- beside a caller's busy stream ----

def test_calls_neither_need_nor_disturb_a_busy_non_blocking_stream(oracle, model):
    """one saca_u32 and one next_tokens call while a caller's non-blocking stream is busy with unrelated copies (the delay chain
    of tests/test_streams.py): the calls answer correctly without that stream having drained -- they never wait on it -- and the
    stream's own work comes out untouched"""
    env = streams.Env()
    hip = env.hip
    S = env.stream()
    try:
        pattern = np.arange(streams.SCRATCH // 8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        assert hip.hipMemcpy(env.scratch[0], pattern.ctypes.data, streams.SCRATCH, streams.H2D) == 0
        assert hip.hipMemset(env.scratch[1], 0, streams.SCRATCH) == 0
        assert hip.hipDeviceSynchronize() == 0
        t = corpus.token_corpus_u32(streams.N, 200000, 31)
        want = reference_suffix_array32(t, oracle)
        ctx = _contexts(model)
        want_next = [next_tokens_definition(model.t, model.lst, c) for c in ctx]

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        got = saca_u32(t)
        assert np.array_equal(got, want)

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        lo, hi, ae, loff, toks, counts = model.built.next_tokens(ctx)
        for q, (wlo, whi, wae, wl) in enumerate(want_next):
            assert (int(lo[q]), int(hi[q]), int(ae[q])) == (wlo, whi, wae) and _listing(loff, toks, counts, q) == wl, q

        assert hip.hipStreamSynchronize(S) == 0
        back = np.empty_like(pattern)
        for p in env.scratch:                                         # an even number of copies each: both buffers hold the pattern
            assert hip.hipMemcpy(back.ctypes.data, p, streams.SCRATCH, streams.D2H) == 0
            assert np.array_equal(back, pattern)
    finally:
        hip.hipStreamSynchronize(S)
        hip.hipStreamDestroy(S)
        env.close()
