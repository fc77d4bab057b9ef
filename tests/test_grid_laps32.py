"""GPU suite for the 32-bit token forms (ids below 2^24) past one launch's grid: tests/test_grid_laps.py
for Sym = uint32_t and the compaction at stride 3.  The sizes follow from the device's CU count and the numbers pinned in
tests/test_grid_laps_abi.py; the helpers -- the lap batch, the expected arrays of a batch, the canaried call and its checks --
are those of tests/test_grid_laps.py, imported.

1. The build past its laps: n = tok32_build_size(cu) tokens is just past one lap of k_tok_be_image3 with a partial last group of
   16 tokens, and its 3 n + 1 byte-level entries lie between one and two laps of k_tok_compact_count / _scatter with a partial
   last span and a partial last tile; the count scan has seven tiles at 256 CUs.  Three text families, chosen by what the second
   lap of the compaction holds (each asserts that from the oracle's byte-level array before anything runs on the device).
2. The range passes on a later lap: an id that is no token in the second iteration of the image pass, in its partial last group,
   and, beside a supplied array, in the second iteration of k_tok_id_range; a supplied array's own range check as the 16-bit
   suite runs it.
3. Queries over three laps and 37 queries of a fourth on a text that uses all three bytes of its tokens: search, next_tokens
   and infgram, the listing cut by `capacity` inside a query of the second lap, and the 16-bit lap batch on both widths.

Every expected value comes from the oracle or from the definitions of tests/test_tokens_abi.py (written over Python ints;
tests/test_tokens32_abi.py pins that they hold at 24 bits), never from the library."""
import functools

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import TokenIndex32
import test_tokens_abi as tokens_abi
from test_grid_laps import (BACKOFF, HOT, PAD, SHARED_STATS, Batch, Expected, TokenModel, TokIndex, check_call, check_capacity_cut, cu_count,
                            raw_query, token_rows)
from test_grid_laps_abi import (TK_IMAGE3_ITEMS, TK_TILE, ngram_waves, tok32_build_size, tok_compact_lap, tok_id_range_lap,
                                tok_image3_lap, tok_range_lap)
from test_tokens32 import CANARY32, CAPS, ERANGE, _saca_u32_canaried, _saca_u32_raw
from test_tokens32_abi import LIMIT, be_image3, every_third_thirded, families32, reference_suffix_array32

pytestmark = pytest.mark.gpu

FAMILIES = ("multiples_of_65536", "below_256", "zipf_200000")
BAD_IDS = (LIMIT, 0xFFFFFFFF)           # the smallest id that is no token, and the largest word


# ---------------------------------------------------------------- 1. the build past its laps ----

@functools.lru_cache(maxsize=None)
def big_texts():
    """families32 at the build size, called once -> the three families used here"""
    every = families32(tok32_build_size(cu_count()))
    return {name: every[name] for name in FAMILIES}


@functools.lru_cache(maxsize=None)
def big_tokens32(family):
    """-> (the text of tok32_build_size tokens, its reference array, the entries the compaction keeps on its second lap, the
    entries of that lap): computed once, shared, never changed.  The reference is reference_suffix_array32's route above
    BRUTE_MAX tokens, which tests/test_tokens32_abi.py pins against brute force."""
    from conftest import Oracle
    cu = cu_count()
    t = big_texts()[family]
    t.setflags(write=False)
    assert t.size == tok32_build_size(cu) > tokens_abi.BRUTE_MAX and t.dtype == np.uint32
    byte_sa = Oracle().sais(be_image3(t))
    assert byte_sa.size == 3 * t.size + 1
    ref = every_third_thirded(byte_sa)
    ref.setflags(write=False)
    second = byte_sa[tok_compact_lap(cu):]
    return t, ref, int(np.count_nonzero(second % 3 == 0)), int(second.size)


@pytest.mark.parametrize("family", FAMILIES)
def test_token32_build_past_its_laps(family):
    """The end of the byte-level array holds the suffixes with the largest first byte.  Under multiples_of_65536 (the two low
    bytes of every token are zero) nearly all of them start at a token: the second lap's counts, their place in the scan and its
    scatter carry the end of the token array.  Under below_256 (the two high bytes are zero) none does: the second lap counts
    zeros and scatters nothing.  Under zipf_200000 every byte varies: mixed tiles."""
    t, ref, kept, second = big_tokens32(family)
    cu = cu_count()
    assert second == 3 * t.size + 1 - tok_compact_lap(cu) > 0 and ref.size == t.size + 1
    if family == "multiples_of_65536":
        assert kept > 0.9 * second and kept > 3 * TK_TILE, (kept, second)
    elif family == "below_256":
        assert kept == 0
    else:
        assert 0.1 * second < kept < 0.9 * second, (kept, second)
    for how, got in (("saca_u32", _saca_u32_canaried(t)), ("index", None)):
        if got is None:
            ix = TokenIndex32(t)
            got = ix.sa()
            ix.close()
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (family, how, int(bad.size), bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())
    st = sa.last_tok_stats()
    assert st["image_ms"] >= 0 and st["build_ms"] > 0 and st["compact_ms"] > 0


# ---------------------------------------------------------------- 2. the range passes on a later lap ----

def create_code(t, arr):
    """sa_amd_tok32_index_create's answer; an index that was made is destroyed at once, nothing is asked of it"""
    try:
        ix = TokenIndex32(t, arr)
    except sa.SuffixArrayError as e:
        return e.code
    ix.close()
    return 0


def id_places(cu, n):
    return {"token_7": 7, "second_lap_of_the_id_range": tok_id_range_lap(cu) + 5, "second_lap_of_the_image": tok_image3_lap(cu) + 5,
            "last_token": n - 1}


@pytest.mark.parametrize("bad_id", BAD_IDS, ids=["2_to_the_24", "ffffffff"])
@pytest.mark.parametrize("where", ["token_7", "second_lap_of_the_id_range", "second_lap_of_the_image", "last_token"])
def test_a_text_id_that_is_no_token_on_a_later_lap(where, bad_id):
    """One id of 2^24 or more: at token 7; at the sixth token of the second iteration of k_tok_id_range; at the sixth token of the
    second iteration of k_tok_be_image3 (its first group there); at the last token, which lies in the image pass's partial last
    group and in a later iteration of both.  The image pass is the guard of sa_amd_saca_u32 and of the index that builds its
    array, k_tok_id_range that of the index created from a supplied array -- the only one between that text and every later
    read of it.  Each answers SA_AMD_ERANGE; saca_u32 leaves its output and the canaries as they were.  No query is run."""
    t, ref, _, _ = big_tokens32("below_256")
    n, cu = t.size, cu_count()
    at = id_places(cu, n)[where]
    assert 0 <= at < n
    if where == "second_lap_of_the_id_range":
        assert tok_id_range_lap(cu) <= at < 2 * tok_id_range_lap(cu)
    if where == "second_lap_of_the_image":
        assert tok_image3_lap(cu) <= at < tok_image3_lap(cu) + TK_IMAGE3_ITEMS
    if where == "last_token":
        assert n % TK_IMAGE3_ITEMS and at >= tok_image3_lap(cu) and at >= tok_id_range_lap(cu)
    bad = t.copy()
    bad[at] = bad_id
    rc, buf = _saca_u32_raw(bad)
    assert rc == ERANGE, (where, rc)
    assert np.all(buf == CANARY32), where
    assert create_code(bad, None) == ERANGE, where
    assert create_code(bad, ref) == ERANGE, where


@pytest.mark.parametrize("where", ["correct", "slot_7", "second_lap", "last_slot", "swapped"])
def test_range_check_of_a_supplied_array_beside_the_id_range_pass(where):
    """the cases of tests/test_grid_laps.py for k_tok_sa_range, on the unmodified text: at this width its flag is shared with
    k_tok_id_range's.  One bad entry (n + 1) in its first lap, one in its second and one in the last slot are each refused with
    -6; entries 0 and 1 swapped (in range, but SA[0] != n) with -1; the reference array is taken.  No query is run."""
    t, ref, _, _ = big_tokens32("below_256")
    n = t.size
    lap = tok_range_lap(cu_count())
    assert 7 < lap and lap + 5 < n
    if where == "correct":
        assert create_code(t, ref) == 0
        return
    bad = ref.copy()
    if where == "swapped":
        bad[0], bad[1] = bad[1], bad[0]
    else:
        bad[{"slot_7": 7, "second_lap": lap + 5, "last_slot": n}[where]] = n + 1
    assert create_code(t, bad) == (-1 if where == "swapped" else ERANGE)


# ---------------------------------------------------------------- 3. queries over three laps at Sym = uint32_t ----

FLIP = 0x010000                         # differs from a present token only in its top byte


def widen(v):
    """a strictly increasing map of the 16-bit tokens into 24 bits whose values use all three bytes; the two edge tokens go to
    the two edge tokens.  Token order, and with it every range and count, carries over."""
    v = int(v)
    return 0 if v == 0 else 0xFFFFFF if v == 0xFFFF else v * 256 + v % 251


class TokIndex32:
    def __init__(self, ix):
        self.ix = ix

    def call(self, batch, capacity, backoff):
        return raw_query(sa.lib().sa_amd_tok32_index_next_tokens, sa.lib().sa_amd_tok32_index_infgram, self.ix._h, batch, np.uint32, capacity,
                         backoff)

    @staticmethod
    def stats():
        return sa.last_tok_stats()


ONLY_MAPPED = (0, 1, 2, 4, 5, 6, 7)     # the kinds whose contexts are TokenModel's with their tokens widened


class Token32Model:
    """TokenModel's text through `widen`, its reference array, ten kinds of context and the lap batch over them.  The kinds
    "absent" and "edge" of the 16-bit model are replaced by contexts that differ from present ones in the top byte of one token
    only; the tenth kind is read from the 3-byte image at offsets that are no multiple of 3."""

    def __init__(self, oracle, narrow):
        self.narrow = narrow
        W = narrow.batch.W
        every = np.arange(65536, dtype=np.int64)
        table = every * 256 + every % 251
        table[0], table[0xFFFF] = 0, 0xFFFFFF
        assert np.all(np.diff(table) > 0) and int(table.max()) < LIMIT and all(widen(v) == table[v] for v in (0, 1, 250, 251, 40000, 65534, 65535))
        self.tok = tok = table[narrow.tok].astype(np.uint32)
        tok.setflags(write=False)
        self.t = t = [int(x) for x in tok]
        self.n = n = len(t)
        assert n == narrow.n > tokens_abi.BRUTE_MAX and 0x000000 in t and 0xFFFFFF in t
        for shift in (0, 8, 16):                                      # all three bytes are used
            assert np.unique((tok >> shift) & 255).size > 8, shift
        self.arr = reference_suffix_array32(tok, oracle)
        self.arr.setflags(write=False)
        assert np.array_equal(self.arr, narrow.arr)                   # (an increasing map: the same order)
        self.lst = lst = self.arr.tolist()
        have = set(t)

        def present(p):
            lo, hi = tokens_abi.range_definition(t, lst, p)
            return hi > lo

        def flipped(p, k):
            q = list(p)
            q[k] ^= FLIP
            assert present(p) and q[k] not in have and 0 <= q[k] < LIMIT, (p, k)
            return q

        mapped = [[[widen(v) for v in p] for p in pool] for pool in narrow.pools]
        short = mapped[2]
        two = next(t[a:a + 3] for a in range(100, n) if len(set(t[a:a + 3])) == 3 and 1 <= self._stripped([t[a + 2]]) <= 64)
        top, zero, hot = 0xFFFFFF, 0x000000, widen(HOT)
        image = be_image3(tok)
        inside = [[(int(image[a + 3 * i]) << 16) | (int(image[a + 3 * i + 1]) << 8) | int(image[a + 3 * i + 2]) for i in range(k)]
                  for a, k in ((1, 1), (101, 2), (5002, 3), (8002, 2))]
        self.pools = [
            mapped[0],                                                # the empty context
            mapped[1],                                                # streamed, more than 256 slots
            short,                                                    # 1 to 64 slots
            # absent by the top byte of the first, the last, a middle token (a back-off of the first and the third ends in a short range)
            [flipped(short[0] if len(short[0]) > 1 else two[1:], 0), flipped([hot, widen(1000)], 1), flipped(two, 1)],
            mapped[4],                                                # the whole text
            mapped[5],                                                # ends the text and occurs elsewhere
            mapped[6],                                                # 600 continuations
            mapped[7],                                                # inside the run
            # tokens 0x000000 and 0xFFFFFF, and what differs from them in the top byte
            [flipped([zero, zero], 0), flipped([top, top], 0), flipped([zero, top, zero], 1), [top, top], [zero, top]],
            inside,                                                   # read from the byte image inside a token
        ]
        assert [len(p) for p in self.pools] == [len(p) for p in narrow.pools]      # the batch has the 16-bit batch's shape
        self.batch = Batch(W, [[np.array(p, dtype=np.uint32) for p in pool] for pool in self.pools], np.uint32)
        assert np.array_equal(self.batch.ids, narrow.batch.ids)
        self.distinct = [p for pool in self.pools for p in pool]
        self._expected, self._rows = {}, {}
        rows = self.rows(None)
        first = np.concatenate(([0], np.cumsum([len(p) for p in self.pools])))
        kinds = [rows[first[k]:first[k + 1]] for k in range(len(self.pools))]
        eff = sa.NGRAM_STREAM_CAP_DEFAULT
        assert kinds[0][0][1:4] == (0, n + 1, 1) and kinds[0][0][6] > eff and 256 < len(kinds[0][0][4]) <= 1500
        assert all(256 < r[6] <= eff for r in kinds[1]) and all(1 <= r[6] <= 64 for r in kinds[2])
        assert all(r[1] == r[2] for r in kinds[3]) and all(r[2] - r[1] == 1 and r[3] == 1 for r in kinds[4])
        assert all(r[3] == 1 and r[6] >= 1 and len(r[4]) == 1 for r in kinds[5])
        assert len(kinds[6][0][4]) == 600 and kinds[6][0][6] == 600 and max(kinds[6][0][4]) > 65535
        assert all(r[6] > 256 and len(r[4]) == 1 for r in kinds[7])
        assert all(r[1] == r[2] for r in kinds[8][:3]) and all(r[2] > r[1] for r in kinds[8][3:])
        assert sum(r[1] == r[2] for r in kinds[9]) >= 2                # the image holds them, no token position does
        for p in inside:
            assert be_image3(p).tobytes() in image.tobytes()
        self.assert_mapped_rows(None)

    def _stripped(self, p):
        lo, hi, ae, _ = tokens_abi.next_tokens_definition(self.t, self.lst, p)
        return hi - lo - ae

    def rows(self, backoff):
        """token_rows on the widened text; the route models' sentinel is sym_end<uint32_t>() = 2^24"""
        if backoff not in self._rows:
            self._rows[backoff] = token_rows(self.t, self.lst, self.distinct, backoff, LIMIT)
        return self._rows[backoff]

    def assert_mapped_rows(self, backoff):
        """for the kinds that were only mapped, the rows are the 16-bit model's rows with their tokens widened"""
        narrow = self.narrow
        mine, theirs = self.rows(backoff), token_rows(narrow.t, narrow.lst, narrow.distinct, backoff)
        first = np.concatenate(([0], np.cumsum([len(p) for p in self.pools])))
        for k in ONLY_MAPPED:
            for a, b in zip(mine[first[k]:first[k + 1]], theirs[first[k]:first[k + 1]]):
                assert a[:4] == b[:4] and a[5:] == b[5:] and a[4] == [widen(v) for v in b[4]], (k, backoff)

    def expected(self, backoff):
        if backoff not in self._expected:
            self.assert_mapped_rows(backoff)
            self._expected[backoff] = Expected(self.batch, self.rows(backoff), np.uint32)
            assert self._expected[backoff].total < 20 << 20
        return self._expected[backoff]


@functools.lru_cache(maxsize=None)
def narrow_model():
    """the 16-bit model of tests/test_grid_laps.py for this device's waves: made once, shared, never changed"""
    from conftest import Oracle
    return TokenModel(Oracle(), ngram_waves(cu_count()))


@pytest.fixture(scope="module")
def token32_model(oracle):
    m = Token32Model(oracle, narrow_model())
    built = TokenIndex32(m.tok)
    m.build_times = {k: sa.last_tok_stats()[k] for k in ("image_ms", "build_ms", "compact_ms")}
    given = TokenIndex32(m.tok, m.arr)
    m.indexes = (("built", TokIndex32(built)), ("given", TokIndex32(given)))
    try:
        yield m
    finally:
        built.close()
        given.close()


def test_token32_search_over_three_laps(token32_model):
    b, exp = token32_model.batch, token32_model.expected(None)
    assert b.count > 3 * b.W
    for name, index in token32_model.indexes:
        has = np.full(b.count + 2 * PAD, 0xA5, dtype=np.uint8)
        lo, hi = np.full(b.count + 2 * PAD, CANARY32, dtype=np.uint32), np.full(b.count + 2 * PAD, CANARY32, dtype=np.uint32)
        assert sa.lib().sa_amd_tok32_index_search(index.ix._h, b.data.ctypes.data, b.off.ctypes.data, b.count, has[PAD:].ctypes.data,
                                                  lo[PAD:].ctypes.data, hi[PAD:].ctypes.data) == 0
        for a in (has, lo, hi):
            raw = a.view(np.uint8)
            assert np.all(raw[:PAD * a.itemsize] == 0xA5) and np.all(raw[(PAD + b.count) * a.itemsize:] == 0xA5), name
        for what, got, want in (("lo", lo, exp.lo), ("hi", hi, exp.hi), ("contains", has, (exp.hi > exp.lo).astype(np.uint8))):
            bad = np.flatnonzero(got[PAD:PAD + b.count] != want)
            assert bad.size == 0, (name, what, int(bad.size), bad[:4].tolist(), [int(q) // b.W for q in bad[:4]])


@pytest.mark.parametrize("cap", CAPS)
def test_next_tokens32_over_three_laps(token32_model, cap):
    exp = token32_model.expected(None)
    for name, index in token32_model.indexes:
        st = check_call(index, token32_model.batch, exp, cap, None, (name, cap))
        assert st["compared_tokens"] == -1
        assert {k: st[k] for k in token32_model.build_times} == token32_model.build_times and st["build_ms"] > 0      # the build's times stay


@pytest.mark.parametrize("cap", CAPS)
def test_token32_infgram_over_three_laps(token32_model, cap):
    for backoff in BACKOFF:
        exp = token32_model.expected(backoff)
        for name, index in token32_model.indexes:
            st = check_call(index, token32_model.batch, exp, cap, backoff, (name, cap, backoff))
            assert st["compared_tokens"] >= 0
            assert {k: st[k] for k in token32_model.build_times} == token32_model.build_times


@pytest.mark.parametrize("backoff", [None, (1, 0)], ids=["next_tokens", "infgram"])
def test_token32_listing_cut_inside_a_query_of_the_second_lap(token32_model, backoff):
    exp = token32_model.expected(backoff)
    for name, index in token32_model.indexes:
        check_capacity_cut(index, token32_model.batch, exp, backoff, (name, backoff))


@pytest.mark.parametrize("cap", CAPS)
def test_the_two_widths_lap_alike(cap):
    """the 16-bit model's own text and lap batch, cast to uint32, on an index of either width: both sides against the definitions
    (TokenModel.expected), their shared counters against each other"""
    m = narrow_model()
    b = m.batch
    wide = Batch(b.W, [[np.asarray(p, dtype=np.uint32) for p in pool] for pool in m.pools], np.uint32)
    assert np.array_equal(wide.ids, b.ids) and np.array_equal(wide.off, b.off) and np.array_equal(wide.data, b.data)
    ix16, ix32 = sa.TokenIndex(m.tok), TokenIndex32(m.tok.astype(np.uint32))
    try:
        for backoff in (None, (2, 0)):
            exp = m.expected(backoff)
            st16 = check_call(TokIndex(ix16), b, exp, cap, backoff, ("uint16", cap, backoff))
            st32 = check_call(TokIndex32(ix32), wide, exp, cap, backoff, ("uint32", cap, backoff))
            for k in SHARED_STATS:
                assert st16[k] == st32[k], (cap, backoff, k, st16[k], st32[k])
            assert st16["compared_tokens"] == st32["compared_tokens"], (cap, backoff)
    finally:
        ix16.close()
        ix32.close()
