"""A byte index and a token index over the same symbols below 256 must agree: the two instantiations of the symbol-generic
query core (kernels/sym.hpp, DESIGN.md sections 21 and 23) pinned to each other -- ranges, back-off, listings, and the work
counters, which are equal by construction (the plain range is the same bisection and chunks of 64 symbols are charged alike).

Text: about 6 000 symbols over {0 .. 7} with planted markers 100, 101, ...; marker k occurs exactly c_k times, each time followed by
a cycling continuation, c_k in {1, 2, 255, 256, 257, 1 024, 1 025}: one streaming trip of NG_LOADS * 64 = 256 slots and the default
stream cap, each with its neighbours.  The byte index has no bucket table and no LCP table, so both indexes take the plain route.
Patterns: empty, the compare's chunk edges (1, 2, 63 .. 65, 127 .. 129 symbols), the whole text with and without one symbol more,
an absent symbol, every marker as a one-symbol context.  Everything under the stream caps 0, default and 2^31 - 1."""
import numpy as np
import pytest

import suffix_array_amd as sa

pytestmark = pytest.mark.gpu

MARKER0 = 100
MARKER_COUNTS = (1, 2, 255, 256, 257, 1024, 1025)
ABSENT = 200
CAPS = (0, -1, 2**31 - 1)               # every non-empty range searched; the default; every range streamed
BACKOFF = ((1, 0), (2, 0), (1, 3))      # (min_count, max_len)
SHARED_STATS = ("patterns", "range_searches", "stream_slots", "search_slots", "stream_queries", "search_queries", "empty_queries",
                "entries", "stream_cap", "backoff", "passes", "readbacks")


def _text():
    rng = np.random.default_rng(41)
    pieces = []
    for k, c in enumerate(MARKER_COUNTS):
        for j in range(c):
            pieces.append([MARKER0 + k, j % 8])
    order = rng.permutation(len(pieces))
    out = []
    for i in order:
        out.extend(pieces[i])
        if rng.integers(0, 8) == 0:                                    # filler: markers are not all two symbols apart
            out.extend(int(v) for v in rng.integers(0, 8, int(rng.integers(1, 4))))
    t = np.array(out, dtype=np.uint8)
    assert 5800 <= t.size <= 6600 and int(t.max()) < ABSENT
    for k, c in enumerate(MARKER_COUNTS):
        assert int(np.count_nonzero(t == MARKER0 + k)) == c
    t.setflags(write=False)
    return t


class Pair:
    """the text and its two indexes; shared by the tests below, never changed"""

    def __init__(self):
        self.t = _text()
        self.n = int(self.t.size)
        self.bytes_ix = sa.DeviceIndex(self.t)                           # (no enable_buckets, no enable_lcp: the plain route)
        self.tok_ix = sa.TokenIndex(self.t.astype(np.uint16))

    def close(self):
        self.bytes_ix.close()
        self.tok_ix.close()

    def patterns(self):
        t, n = self.t.tolist(), self.n
        rng = np.random.default_rng(43)
        pats = [[], list(t), list(t) + [3], [ABSENT]]
        for k in (1, 2, 63, 64, 65, 127, 128, 129):
            a = int(rng.integers(0, n - k))
            pats.append(t[a:a + k])
            pats.append(t[n - k:])                                      # a suffix of the text: at_end
        return pats + [[MARKER0 + k] for k in range(len(MARKER_COUNTS))]

    def prompts(self):
        t, n = self.t.tolist(), self.n
        rng = np.random.default_rng(47)
        out = self.patterns() + [[ABSENT, MARKER0 + 3], [ABSENT] + t[40:45]]
        for k in (2, 5, 20, 70, 130):
            a = int(rng.integers(0, n - k))
            out.append([ABSENT] + t[a + 1:a + k])                       # the first symbol breaks the match: a shorter suffix
            out.append(t[a:a + k] + [ABSENT])                           # the last one does: the empty suffix
        return out


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    try:
        yield p
    finally:
        p.close()


def _as_bytes(pats):
    return [bytes(p) for p in pats]


def _as_tokens(pats):
    return [np.array(p, dtype=np.uint16) for p in pats]


def _stats_agree(where):
    b, t = sa.last_ngram_stats(), sa.last_tok_stats()
    for k in SHARED_STATS:
        assert b[k] == t[k], (where, k, b[k], t[k])
    assert b["compared_bytes"] == t["compared_tokens"], (where, b["compared_bytes"], t["compared_tokens"])
    return b


def _results_agree(where, got_b, got_t):
    names = ("suffix_len", "lo", "hi", "at_end", "list_off", "symbols", "counts")[-len(got_b):]
    for name, x, y in zip(names, got_b, got_t):
        assert x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64)), (where, name)


def test_same_suffix_array(pair):
    assert np.array_equal(pair.bytes_ix.suffix_array(), pair.tok_ix.sa())


def test_search_ranges_agree(pair):
    pats = pair.patterns()
    b = pair.bytes_ix.search(_as_bytes(pats))
    lo, hi = pair.tok_ix.search(_as_tokens(pats))
    assert np.array_equal(b["lo"], lo) and np.array_equal(b["hi"], hi)
    assert int(hi[0]) - int(lo[0]) == pair.n + 1 and hi[1] - lo[1] == 1 and hi[2] == lo[2] and hi[3] == lo[3]
    assert (hi[-len(MARKER_COUNTS):] - lo[-len(MARKER_COUNTS):]).tolist() == list(MARKER_COUNTS)


@pytest.mark.parametrize("cap", CAPS)
def test_continuations_agree(pair, cap):
    pats = pair.patterns()
    prev = sa.ngram_set_stream_cap(cap)
    try:
        got_b = pair.bytes_ix.next_bytes(_as_bytes(pats))
        got_t = pair.tok_ix.next_tokens(_as_tokens(pats))
        _results_agree(cap, got_b, got_t)
        st = _stats_agree(cap)
        assert st["patterns"] == len(pats) and st["passes"] == 2 and st["readbacks"] == 1 and st["compared_bytes"] == -1
        lo, hi, ae = (x.astype(np.int64) for x in got_b[:3])
        cnt = hi - lo - ae
        limit = sa.NGRAM_STREAM_CAP_DEFAULT if cap == -1 else cap
        assert st["stream_cap"] == limit and MARKER_COUNTS[-2] == sa.NGRAM_STREAM_CAP_DEFAULT     # 1 024 streamed, 1 025 searched
        assert st["empty_queries"] == int(np.count_nonzero(cnt == 0)) > 0
        assert st["stream_queries"] == int(np.count_nonzero((cnt > 0) & (cnt <= limit)))
        assert st["search_queries"] == int(np.count_nonzero(cnt > limit)) and (cap != -1 or st["search_queries"] >= 2)
        assert st["stream_slots"] == int(cnt[(cnt > 0) & (cnt <= limit)].sum())
    finally:
        sa.ngram_set_stream_cap(prev)


@pytest.mark.parametrize("cap", CAPS)
def test_backoff_agrees(pair, cap):
    prompts = pair.prompts()
    prev = sa.ngram_set_stream_cap(cap)
    try:
        for min_count, max_len in BACKOFF:
            got_b = pair.bytes_ix.infgram(_as_bytes(prompts), min_count, max_len)
            got_t = pair.tok_ix.infgram(_as_tokens(prompts), min_count, max_len)
            _results_agree((cap, min_count, max_len), got_b, got_t)
            st = _stats_agree((cap, min_count, max_len))
            assert st["backoff"] == 1 and st["readbacks"] == 1 and st["compared_bytes"] > 0 and st["range_searches"] > 0
            s = got_b[0]
            assert int(s.min()) == 0 and (min_count > 1 or int(s.max()) == (pair.n if max_len == 0 else max_len))
    finally:
        sa.ngram_set_stream_cap(prev)
