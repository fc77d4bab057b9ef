"""GPU suite for the 16-bit token texts: sa_amd_saca_u16 against the CPU reference on every text family at
the sizes where the construction changes its path, the token index (built on the device and created from the reference array)
against the definitions of tests/test_tokens_abi.py -- search, next_tokens and infgram with the stream cap forced to 0, at its
default and at 2^31 - 1 --, canaries around every output buffer, and both kinds of call beside a caller's busy non-blocking stream.

Sizes.  Construction: 2 n around the 8 192-byte small-text route of the byte builder (n = 4 095 .. 4 097), n + 1 and 2 n + 1 around
one compaction tile (2 048 entries) and one span of four tiles, and n = 70 001 (the general route, many tiles); brute force is the
reference up to 2 000 tokens, the oracle on the big-endian image above (the CPU suite pins that the two agree).  Index: 7 200
tokens -- the empty context's range is above the default stream cap of 1 024, a planted token has 600 distinct continuations."""
import ctypes

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
import test_streams as streams
from test_tokens_abi import (BRUTE_MAX, EXAMPLE_SA, EXAMPLE_TEXT, SPAN, TILE, as_tokens, be_image, families, infgram_definition,
                             next_tokens_definition, range_definition, reference_suffix_array)

pytestmark = pytest.mark.gpu

CANARY32 = 0xA5A5A5A5
PAD = 16                                # canary words on either side of an output
BUILD_SIZES = sorted({0, 1, 2, 3, 4095, 4096, 4097,
                      TILE // 2 - 1, TILE // 2,                                   # 2 n + 1 one below and one above a tile
                      TILE - 2, TILE - 1, TILE,                                   # n + 1 at a tile
                      SPAN * TILE // 2 - 1, SPAN * TILE // 2,                     # 2 n + 1 around a span of tiles
                      SPAN * TILE - 2, SPAN * TILE - 1, SPAN * TILE,              # n + 1 at a span
                      70001})
CAPS = (0, -1, 2**31 - 1)               # every non-empty range searched; the default; every range streamed
HOT = 40000                             # the planted token of the index text: 600 distinct continuations


def _saca_u16_canaried(t):
    """sa_amd_saca_u16 through the library with canary words around the output"""
    buf = np.full(t.size + 1 + 2 * PAD, CANARY32, dtype=np.uint32)
    rc = sa.lib().sa_amd_saca_u16(t.ctypes.data if t.size else None, buf[PAD:].ctypes.data, t.size)
    assert rc == 0, rc
    assert np.all(buf[:PAD] == CANARY32) and np.all(buf[PAD + t.size + 1:] == CANARY32)
    return buf[PAD:PAD + t.size + 1].copy()


@pytest.mark.parametrize("n", BUILD_SIZES)
def test_saca_u16_against_the_reference(oracle, n):
    for name, t in families(n).items():
        got = _saca_u16_canaried(t)
        want = reference_suffix_array(t, oracle)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, n, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert np.array_equal(sa.saca_u16(t), want), (name, n)
    st = sa.last_tok_stats()
    assert n == 0 or (st["image_ms"] >= 0 and st["build_ms"] > 0 and st["compact_ms"] > 0)


def test_header_example_and_endianness():
    """the text that a little-endian image orders differently"""
    assert sa.saca_u16(EXAMPLE_TEXT).tolist() == EXAMPLE_SA
    assert sa.saca_u16(np.array([0x0100, 0x0001], dtype=np.uint16)).tolist() == [2, 1, 0]
    assert sa.saca_u16([]).tolist() == [0]


# ---------------------------------------------------------------- the index ----

class Model:
    """the index text, its reference array and the two indexes; shared by the tests below, never changed"""

    def __init__(self, oracle):
        planted = np.empty(1200, dtype=np.uint16)
        planted[0::2] = HOT
        planted[1::2] = 1000 + np.arange(600)
        body = corpus.token_corpus(6000, 50000, 9)
        self.tok = as_tokens(np.concatenate((body[:3000], planted, body[3000:])))
        self.tok.setflags(write=False)
        self.t = [int(x) for x in self.tok]
        self.n = len(self.t)
        assert self.n > BRUTE_MAX
        self.arr = reference_suffix_array(self.tok, oracle)
        self.arr.setflags(write=False)
        self.lst = self.arr.tolist()
        self.built = sa.TokenIndex(self.tok)
        self.given = sa.TokenIndex(self.tok, self.arr)
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


def _odd_offset_patterns(m):
    """tokens read from the byte image at ODD offsets: they occur in the image, but a match there starts inside a token"""
    b = be_image(m.tok)
    out = []
    for a in (1, 101, 2001, 6001):
        for k in (1, 2, 3):
            raw = b[a:a + 2 * k]
            out.append([(int(raw[2 * i]) << 8) | int(raw[2 * i + 1]) for i in range(k)])
    return out


def _search_patterns(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(17)
    pats = [[], list(t), list(t) + [5], [HOT], [HOT, 1000], [HOT, 999], [65535, 65535], [0]]
    for k in (1, 2, 5, 63, 64, 65, 66, 128, 129):                     # around the 64 tokens of a wave step
        a = int(rng.integers(0, n - k))
        pats.append(t[a:a + k])
        pats.append(t[a:a + k - 1] + [(t[a + k - 1] + 1) & 0xFFFF])    # differs in its last token
        pats.append(t[n - k:])                                        # a suffix of the text
    return pats + _odd_offset_patterns(m)


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
    odd = _odd_offset_patterns(model)
    image = be_image(model.tok).tobytes()
    empty = 0
    for p in odd:
        assert be_image(as_tokens(p)).tobytes() in image              # the byte image holds it ...
        lo, hi = range_definition(model.t, model.lst, p)
        empty += lo == hi                                             # ... but no token position does
    assert empty >= len(odd) // 2
    lo, hi = model.built.search([])
    assert lo.size == 0 and hi.size == 0


def _contexts(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(23)
    ctx = [[], [HOT], [HOT, 1000], t[n - 2:], t[n - 1:], list(t), [9, 9, 9], [HOT, 999]]
    for k in (1, 1, 1, 2, 2, 3, 7, 64, 65):
        a = int(rng.integers(0, n - k))
        ctx.append(t[a:a + k])
    top = int(np.bincount(m.tok).argmax())                            # the most frequent token of the corpus part
    return ctx + [[top]]


def _prompts(m):
    t, n = m.t, m.n
    rng = np.random.default_rng(29)
    out = [[], [7], [7, HOT], list(t[n - 5:]), [3, 3] + t[100:110], t[200:330]]
    for k in (2, 5, 20):
        a = int(rng.integers(0, n - k))
        out.append([(t[a] + 1) & 0xFFFF] + t[a + 1:a + k])            # the first token breaks the match: a shorter suffix
        out.append(t[a:a + k] + [(t[a + k - 1] + 7) & 0xFFFF])
    return out


def _listing(loff, toks, counts, q):
    return [(int(a), int(b)) for a, b in zip(toks[loff[q]:loff[q + 1]], counts[loff[q]:loff[q + 1]])]


@pytest.mark.parametrize("cap", CAPS)
def test_next_tokens_against_the_definition(model, cap):
    ctx = _contexts(model)
    want = [next_tokens_definition(model.t, model.lst, c) for c in ctx]
    assert max(len(w[3]) for w in want) > 256 and 600 <= len(want[1][3]) and want[1][1] - want[1][0] <= 1024     # listings beyond 256 entries
    assert want[3][2] == 1 and want[0][2] == 1                                   # at_end
    prev = sa.ngram_set_stream_cap(cap)
    try:
        for name, ix in model.indexes:
            lo, hi, ae, loff, toks, counts = ix.next_tokens(ctx)
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
        ix = sa.TokenIndex(EXAMPLE_TEXT, arr)
        lo, hi, ae, loff, toks, counts = ix.next_tokens([[256, 1], [1], [2], [], [9]])
        assert list(zip(lo.tolist(), hi.tolist()))[:4] == [(4, 6), (1, 3), (3, 4), (0, 6)] and lo[4] == hi[4]
        assert ae.tolist() == [0, 0, 1, 1, 0]
        assert [_listing(loff, toks, counts, q) for q in range(5)] == [[(2, 1), (256, 1)], [(2, 1), (256, 1)], [], [(1, 2), (2, 1), (256, 2)], []]
        for (min_count, max_len), want in (((1, 0), (2, 4, 6)), ((3, 0), (0, 0, 6)), ((2, 1), (1, 1, 3))):
            s, lo, hi = ix.infgram([[7, 256, 1]], min_count, max_len)[:3]
            assert (int(s[0]), int(lo[0]), int(hi[0])) == want
        ix.close()


def test_sub_range_identity(model):
    """the range of context + t is the slice the listing implies"""
    for ctx in ([], [HOT], model.t[50:51]):
        lo, hi, ae, loff, toks, counts = model.built.next_tokens([ctx])
        longer = [ctx + [int(v)] for v in toks]
        slo, shi = model.built.search(longer)
        starts = int(lo[0]) + int(ae[0]) + np.concatenate(([0], np.cumsum(counts.astype(np.int64))[:-1]))
        assert np.array_equal(slo.astype(np.int64), starts) and np.array_equal(shi.astype(np.int64), starts + counts)
        assert int(starts[-1] + counts[-1]) == int(hi[0])


def _raw_query(ix, pats, capacity, backoff, outputs=True):
    """the library call itself with canaried output buffers -> (rc, total, dict of the arrays)"""
    data, off, cnt = sa._token_batch(pats)
    L = sa.lib()

    def buf(count, dtype):
        a = np.empty(count + 2 * PAD, dtype=dtype)
        a.view(np.uint8)[:] = 0xA5
        return a

    out = {"slen": buf(cnt, np.uint32), "lo": buf(cnt, np.uint32), "hi": buf(cnt, np.uint32), "ae": buf(cnt, np.uint8),
           "loff": buf(cnt + 1, np.int64), "toks": buf(max(capacity, 0), np.uint16), "counts": buf(max(capacity, 0), np.uint32)}
    ptr = {k: (v[PAD:].ctypes.data if outputs else None) for k, v in out.items()}
    total = ctypes.c_int64(-7)
    tp = ctypes.byref(total) if outputs else None
    if backoff:
        rc = L.sa_amd_tok_index_infgram(ix._h, data.ctypes.data, off.ctypes.data, cnt, 1, 0, ptr["slen"], ptr["lo"], ptr["hi"], ptr["ae"],
                                        ptr["loff"], ptr["toks"], ptr["counts"], capacity, tp)
    else:
        rc = L.sa_amd_tok_index_next_tokens(ix._h, data.ctypes.data, off.ctypes.data, cnt, ptr["lo"], ptr["hi"], ptr["ae"], ptr["loff"],
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
    pats = _search_patterns(model)[:10]
    data, off, cnt = sa._token_batch(pats)
    want = [range_definition(model.t, model.lst, p) for p in pats]
    has = np.full(cnt + 2 * PAD, 0xA5, dtype=np.uint8)
    lo, hi = np.full(cnt + 2 * PAD, CANARY32, dtype=np.uint32), np.full(cnt + 2 * PAD, CANARY32, dtype=np.uint32)
    L = sa.lib()
    assert L.sa_amd_tok_index_search(model.given._h, data.ctypes.data, off.ctypes.data, cnt, has[PAD:].ctypes.data, lo[PAD:].ctypes.data,
                                     hi[PAD:].ctypes.data) == 0
    assert all(_canaries_hold(a, cnt) for a in (has, lo, hi))
    assert list(zip(lo[PAD:PAD + cnt].tolist(), hi[PAD:PAD + cnt].tolist())) == want
    assert has[PAD:PAD + cnt].tolist() == [int(b > a) for a, b in want]
    assert L.sa_amd_tok_index_search(model.given._h, data.ctypes.data, off.ctypes.data, cnt, None, None, None) == 0
    assert L.sa_amd_tok_index_search(model.given._h, data.ctypes.data, off.ctypes.data, 0, None, None, None) == 0


def test_a_supplied_array_is_range_checked(model):
    bad = model.arr.copy()
    bad[model.n // 2] = model.n + 1                                   # an entry above n
    with pytest.raises(sa.SuffixArrayError) as e:
        sa.TokenIndex(model.tok, bad)
    assert e.value.code == -6
    bad = model.arr.copy()
    bad[0], bad[1] = bad[1], bad[0]                                   # in range, but SA[0] != n
    with pytest.raises(sa.SuffixArrayError) as e:
        sa.TokenIndex(model.tok, bad)
    assert e.value.code == -1
    wrong = np.roll(model.arr[1:], 5)                                 # in range and wrong: unspecified answers, nothing out of range
    ix = sa.TokenIndex(model.tok, np.concatenate((model.arr[:1], wrong)).astype(np.uint32))
    for cap in CAPS:
        prev = sa.ngram_set_stream_cap(cap)
        try:
            lo, hi, ae, loff, toks, counts = ix.next_tokens(_contexts(model))
            assert loff[-1] == toks.size == counts.size and np.all(hi <= model.n + 1)
            ix.infgram(_prompts(model), 2, 0)
        finally:
            sa.ngram_set_stream_cap(prev)
    ix.close()


# ---------------------------------------------------------------- beside a caller's busy stream ----

def test_calls_neither_need_nor_disturb_a_busy_non_blocking_stream(oracle, model):
    """one saca_u16 and one next_tokens call while a caller's non-blocking stream is busy with unrelated copies (the delay chain
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
        t = as_tokens(corpus.token_corpus(streams.N, 50000, 31))
        want = reference_suffix_array(t, oracle)
        ctx = _contexts(model)
        want_next = [next_tokens_definition(model.t, model.lst, c) for c in ctx]

        env.queue_chain(S)
        assert hip.hipStreamQuery(S) == streams.HIP_NOT_READY, "the delay chain is too short: S has drained before the call"
        got = sa.saca_u16(t)
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
