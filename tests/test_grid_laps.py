"""GPU suite for batches and token builds larger than one launch's grid (testing notes: laps).  The query engines and
the token build launch at most cu_count() * c workgroups; a wave, or a workgroup, then loops over the work items it was not given
first.  Every other test of these kernels stays inside the first pass; here the loop step, the state carried from one item to
the next (the LDS table of k_next_bytes, carry / pend / listed / first_at / mine of k_tok_next, the counters of a wave and their
one flush) and the second tile of the offsets' scan run at the sizes where the product library really laps.

Sizes follow from the device's CU count and the numbers pinned in tests/test_grid_laps_abi.py; no literal of one machine.  A
lap batch (lap_batch there) has three full laps and 37 queries of a fourth: 3 W + 37 queries, W = CU * 64 waves, built so that a
wave meets every ordered pair of kinds of query on consecutive laps.  The definitions are computed once per DISTINCT query with
the CPU definitions of the *_abi files and spread over the batch with numpy indexing.

1. byte index: next_bytes and infgram; 2. token index: search, next_tokens, infgram; 3. byte against token on one batch;
4. documents: units, listing entries and patterns past their caps; 5. the token build past one compaction lap, and the range
check of a caller's array on its second lap."""
import contextlib
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
import test_ngram_abi as ngram_abi
import test_tokens_abi as tokens_abi
import test_docs_abi as docs_abi
import test_doc_tf_abi as doc_tf_abi
from test_docs import english, random_table, raw_list
from test_doc_tf import raw_tf, raw_topk
from test_tokens import CAPS, _saca_u16_canaried
from test_grid_laps_abi import (DOC_SCAN_TILE, LAPS, TAIL, TK_TILE, backoff_model, doc_tf_lanes, docs_waves, gather, lap_batch, ngram_waves,
                                pool_of, tok_build_size, tok_compact_lap, tok_range_lap)

pytestmark = pytest.mark.gpu

PAD = 16                                # canary elements on either side of an output
BACKOFF = ((1, 0), (2, 0), (3, 4))      # (min_count, max_len)
PLANT, RUN = 0xF0, 0xFA                 # bytes the English text does not have: followed by all 256 values / a run of 700
RUN_LEN = 700
HOT, TOK_RUN = 40000, 30000             # the same two of the token text: 600 continuations / a run of 700
SHARED_STATS = ("patterns", "range_searches", "stream_slots", "search_slots", "stream_queries", "search_queries", "empty_queries",
                "entries", "stream_cap", "backoff", "passes", "readbacks")


@functools.lru_cache(maxsize=None)
def cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked for in a process of its own: torch brings its own HIP
    runtime, which has to be the first one a process loads (tests/test_score.py), and this one has loaded the library's"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    cu = int(out.stdout.strip().splitlines()[-1])
    assert cu >= 2                                                    # (ten kinds of query need W >= 100 waves)
    return cu


def effective_cap(cap):
    return sa.NGRAM_STREAM_CAP_DEFAULT if cap < 0 else min(cap, 2**31 - 1)


# ---------------------------------------------------------------- a lap batch and what the definitions say of it ----

class Batch:
    """the lap batch over `pools` (per kind its variants: 1-D arrays of symbols) for W waves: ids[q] = the distinct query of q,
    and the flat pattern arrays the library takes"""

    def __init__(self, W, pools, dtype):
        self.W, self.dtype = W, dtype
        sizes = np.array([len(p) for p in pools], dtype=np.int64)
        first = np.concatenate(([0], np.cumsum(sizes)))
        self.kind, variant = lap_batch(W, int(sizes.max()), len(pools))
        self.ids = first[self.kind] + variant % sizes[self.kind]
        self.distinct = [np.asarray(p, dtype=dtype) for pool in pools for p in pool]
        assert np.array_equal(np.unique(self.ids), np.arange(len(self.distinct)))      # every distinct query is asked
        self.off, data = gather(*pool_of(self.distinct, dtype), self.ids)
        self.data = np.ascontiguousarray(data) if data.size else np.zeros(1, dtype=dtype)
        self.count = int(self.ids.size)
        assert self.count == LAPS * W + TAIL


class Expected:
    """rows: per distinct query (s, lo, hi, at_end, symbols, counts, cnt, search_probes, backoff_probes) -> the arrays of the
    whole batch.  cnt: the slots of the stripped range; search_probes: what the boundary-search route probes on it."""

    def __init__(self, batch, rows, sym_dtype):
        ids = batch.ids
        col = lambda k, dtype: np.array([r[k] for r in rows], dtype=dtype)[ids]      # noqa: E731
        self.s, self.lo, self.hi, self.ae = col(0, np.uint32), col(1, np.uint32), col(2, np.uint32), col(3, np.uint8)
        self.loff, self.syms = gather(*pool_of([r[4] for r in rows], sym_dtype), ids)
        loff2, self.counts = gather(*pool_of([r[5] for r in rows], np.uint32), ids)
        assert np.array_equal(self.loff, loff2)
        self.total = int(self.loff[-1])
        self.cnt, self.search_probes, self.backoff_probes = col(6, np.int64), col(7, np.int64), col(8, np.int64)
        self.count = int(ids.size)

    def stats(self, cap, backoff):
        """the counters of a call under stream cap `cap`, from the route models summed over the batch"""
        eff = effective_cap(cap)
        stream, search = (self.cnt > 0) & (self.cnt <= eff), self.cnt > eff
        return {"patterns": self.count, "range_searches": int(self.backoff_probes.sum()) if backoff else self.count,
                "stream_slots": int(self.cnt[stream].sum()), "search_slots": int(self.search_probes[search].sum()),
                "stream_queries": int(stream.sum()), "search_queries": int(search.sum()), "empty_queries": int((self.cnt == 0).sum()),
                "entries": self.total, "stream_cap": eff, "backoff": int(bool(backoff)), "passes": 2, "readbacks": 1}


def raw_query(next_fn, infgram_fn, handle, batch, sym_dtype, capacity, backoff):
    """the library call itself on the flat pattern arrays, canaries around every output -> (total, the padded buffers)"""
    cnt = batch.count

    def buf(k, dtype):
        a = np.empty(k + 2 * PAD, dtype=dtype)
        a.view(np.uint8)[:] = 0xA5
        return a

    out = {"s": buf(cnt, np.uint32), "lo": buf(cnt, np.uint32), "hi": buf(cnt, np.uint32), "ae": buf(cnt, np.uint8),
           "loff": buf(cnt + 1, np.int64), "syms": buf(capacity, sym_dtype), "counts": buf(capacity, np.uint32)}
    ptr = {k: v[PAD:].ctypes.data for k, v in out.items()}
    total = ctypes.c_int64(-7)
    tail = (ptr["lo"], ptr["hi"], ptr["ae"], ptr["loff"], ptr["syms"], ptr["counts"], capacity, ctypes.byref(total))
    if backoff:
        rc = infgram_fn(handle, batch.data.ctypes.data, batch.off.ctypes.data, cnt, backoff[0], backoff[1], ptr["s"], *tail)
    else:
        rc = next_fn(handle, batch.data.ctypes.data, batch.off.ctypes.data, cnt, *tail)
    assert rc == 0, rc
    return int(total.value), out


def check_outputs(total, out, exp, capacity, backoff, W, what):
    """every per-query output, every listing entry that fits `capacity`, and nothing outside: the canaries before every buffer,
    behind its used part, and behind `capacity`"""
    assert total == exp.total, (what, total, exp.total)
    wr = min(capacity, exp.total)
    used = {"s": exp.count if backoff else 0, "lo": exp.count, "hi": exp.count, "ae": exp.count, "loff": exp.count + 1, "syms": wr, "counts": wr}
    want = {"s": exp.s, "lo": exp.lo, "hi": exp.hi, "ae": exp.ae, "loff": exp.loff, "syms": exp.syms[:wr], "counts": exp.counts[:wr]}
    for name, a in out.items():
        raw, w = a.view(np.uint8), a.itemsize
        assert np.all(raw[:PAD * w] == 0xA5) and np.all(raw[(PAD + used[name]) * w:] == 0xA5), (what, name, "canary")
        if used[name]:
            got = a[PAD:PAD + used[name]]
            bad = np.flatnonzero(got != want[name])
            if bad.size and name in ("syms", "counts"):                # an entry -> its query
                where = (np.searchsorted(exp.loff, bad[:4], "right") - 1).tolist()
            else:
                where = bad[:4].tolist()
            assert bad.size == 0, (what, name, int(bad.size), "queries", where, "laps", [q // W for q in where],
                                   got[bad[:4]].tolist(), want[name][bad[:4]].tolist())


def check_call(index, batch, exp, cap, backoff, what):
    """one call under stream cap `cap` with room for the whole listing: outputs and counters"""
    prev = sa.ngram_set_stream_cap(cap)
    try:
        total, out = index.call(batch, exp.total + 3, backoff)
        st = index.stats()
    finally:
        sa.ngram_set_stream_cap(prev)
    check_outputs(total, out, exp, exp.total + 3, backoff, batch.W, what)
    want = exp.stats(cap, backoff)
    assert st["stream_queries"] + st["search_queries"] + st["empty_queries"] == batch.count, (what, st)
    assert {k: st[k] for k in want} == want, (what, st, want)
    return st


def check_capacity_cut(index, batch, exp, backoff, what):
    """`capacity` cut inside the listing of a query of the second lap: nothing behind it is written, the total is still reported"""
    W = batch.W
    lens = np.diff(exp.loff)
    inside = W + np.flatnonzero(lens[W:2 * W] >= 2)
    assert inside.size
    q = int(inside[inside.size // 2])
    capacity = int(exp.loff[q] + lens[q] // 2)
    assert exp.loff[q] < capacity < exp.loff[q + 1] and W <= q < 2 * W and capacity < exp.total
    total, out = index.call(batch, capacity, backoff)
    check_outputs(total, out, exp, capacity, backoff, W, what)
    assert index.stats()["passes"] == 2 and index.stats()["entries"] == exp.total


# ---------------------------------------------------------------- 1. the byte index ----

def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


class ByteIndex:
    def __init__(self, ix):
        self.ix = ix

    def call(self, batch, capacity, backoff):
        return raw_query(sa.lib().sa_amd_index_next_bytes, sa.lib().sa_amd_index_infgram, self.ix._h, batch, np.uint8, capacity, backoff)

    @staticmethod
    def stats():
        return sa.last_ngram_stats()


class ByteModel:
    """the byte text, its suffix array, the eight kinds of context, the lap batch over them and the definitions' answers;
    shared by the tests below, never changed"""

    def __init__(self, oracle, W):
        eng = corpus.english_corpus(6000, 5).tobytes()
        assert PLANT not in eng and RUN not in eng
        planted = b"".join(bytes([PLANT, v]) for v in range(256))
        self.tb = tb = eng[:3000] + planted + eng[3000:] + bytes([RUN]) * RUN_LEN      # the run ends the text: one continuation
        self.n = n = len(tb)
        self.t = _u8(tb)
        self.arr = arr = oracle.sais(self.t)
        self.arr.setflags(write=False)

        def stripped(p):
            lo, hi, ae, _ = ngram_abi.next_bytes_definition(tb, arr, p)
            return hi - lo - ae

        grams = sorted({tb[a:a + k] for k in (1, 2) for a in range(0, 6000, 7)})
        streamed = sorted((stripped(g), g) for g in grams if 256 < stripped(g) <= sa.NGRAM_STREAM_CAP_DEFAULT)
        short = [p for p in (tb[100:104], tb[1000:1003], tb[4000:4005], tb[200:230]) if 1 <= stripped(p) <= 64]
        assert len(streamed) >= 2 and len(short) >= 3
        run = bytes([RUN])
        self.pools = [
            [b""],                                                    # the empty context: a range above the default stream cap
            [streamed[0][1], streamed[len(streamed) // 2][1], streamed[-1][1]],       # streamed, more than 256 slots: several trips
            short,                                                    # 1 to 64 slots
            [b"\x01\x02nope", b"zq\x00zq", bytes([RUN, 0])],          # absent
            [tb, tb[1:], tb[7:]],                                     # the whole text: at_end and nothing left
            [run * (RUN_LEN - 1), run * (RUN_LEN - 10), run * (RUN_LEN - 64)],        # ends the text and occurs elsewhere
            [bytes([PLANT])],                                         # 256 continuations
            [run * 2, run * 3, run * 65, run * 300],                  # inside the run: a long range, one continuation
        ]
        self.batch = Batch(W, [[_u8(p) for p in pool] for pool in self.pools], np.uint8)
        self.distinct = [p for pool in self.pools for p in pool]
        self._expected = {}
        self._shape_of_the_kinds()

    def _row(self, p, backoff):
        tb, arr = self.tb, self.arr
        if backoff:
            s, lo, hi, ae, nxt, probes = ngram_abi.infgram_definition(tb, arr, p, *backoff)
        else:
            (lo, hi, ae, nxt), s, probes = ngram_abi.next_bytes_definition(tb, arr, p), len(p), 0
        b, c = ngram_abi.listing_of(nxt)
        cnt = hi - lo - ae
        run = self.t[np.asarray(arr[lo + ae:hi], dtype=np.int64) + s] if cnt else None
        if cnt:
            got, slots = ngram_abi.stream_route_model(run)
            assert np.array_equal(got, nxt) and slots == cnt
            got, searched = ngram_abi.search_route_model(run)
            assert np.array_equal(got, nxt)
        return (s, lo, hi, ae, b, c, cnt, searched if cnt else 0, probes)

    def expected(self, backoff):
        if backoff not in self._expected:
            self._expected[backoff] = Expected(self.batch, [self._row(bytes(p), backoff) for p in self.distinct], np.uint8)
        return self._expected[backoff]

    def _shape_of_the_kinds(self):
        """the kinds are what they are named for"""
        rows = [[self._row(bytes(p), None) for p in pool] for pool in self.pools]
        eff, n = sa.NGRAM_STREAM_CAP_DEFAULT, self.n
        assert rows[0][0][1:4] == (0, n + 1, 1) and rows[0][0][6] > eff
        assert all(4 * 64 < r[6] <= eff for r in rows[1]) and all(1 <= r[6] <= 64 for r in rows[2])
        assert all(r[1] == r[2] and r[6] == 0 for r in rows[3])
        assert all(r[2] - r[1] == 1 and r[3] == 1 and r[6] == 0 for r in rows[4])
        assert all(r[3] == 1 and r[6] >= 1 and len(r[4]) == 1 for r in rows[5])
        assert len(rows[6][0][4]) == 256 and rows[6][0][6] == 257
        assert all(r[6] > 256 and len(r[4]) == 1 for r in rows[7]) and rows[7][0][6] == RUN_LEN - 2


@pytest.fixture(scope="module")
def byte_model(oracle):
    m = ByteModel(oracle, ngram_waves(cu_count()))
    plain = sa.DeviceIndex(m.t, m.arr)
    tables = sa.DeviceIndex(m.t, m.arr)
    tables.buckets()
    tables.enable_lcp()
    m.indexes = (("plain", ByteIndex(plain)), ("bkt_lcp", ByteIndex(tables)))
    try:
        yield m
    finally:
        plain.close()
        tables.close()


@pytest.mark.parametrize("cap", CAPS)
def test_next_bytes_over_three_laps(byte_model, cap):
    exp = byte_model.expected(None)
    assert exp.count > 3 * byte_model.batch.W and exp.count + 1 > 3 * DOC_SCAN_TILE      # the offsets' scan has more than one tile
    for name, index in byte_model.indexes:
        st = check_call(index, byte_model.batch, exp, cap, None, (name, cap))
        assert st["compared_bytes"] == -1


@pytest.mark.parametrize("cap", CAPS)
def test_infgram_over_three_laps(byte_model, cap):
    for backoff in BACKOFF:
        exp = byte_model.expected(backoff)
        for name, index in byte_model.indexes:
            st = check_call(index, byte_model.batch, exp, cap, backoff, (name, cap, backoff))
            assert st["compared_bytes"] >= 0


@pytest.mark.parametrize("backoff", [None, (1, 0)], ids=["next_bytes", "infgram"])
def test_byte_listing_cut_inside_a_query_of_the_second_lap(byte_model, backoff):
    exp = byte_model.expected(backoff)
    for name, index in byte_model.indexes:
        check_capacity_cut(index, byte_model.batch, exp, backoff, (name, backoff))


# ---------------------------------------------------------------- 2. the token index ----

class TokIndex:
    def __init__(self, ix):
        self.ix = ix

    def call(self, batch, capacity, backoff):
        return raw_query(sa.lib().sa_amd_tok_index_next_tokens, sa.lib().sa_amd_tok_index_infgram, self.ix._h, batch, np.uint16, capacity, backoff)

    @staticmethod
    def stats():
        return sa.last_tok_stats()


def token_rows(t, lst, distinct, backoff, end=tokens_abi.END):
    """per distinct token query the row Expected takes, from the definitions and route models of tests/test_tokens_abi.py.  The
    back-off is the bisection (backoff_model), which tests/test_grid_laps_abi.py pins to the definition that tries every length.
    end: the route models' sentinel, sym_end<Sym>() of the index's token type."""
    rows = []
    for p in distinct:
        p = [int(x) for x in p]
        s, probes = len(p), 0
        if backoff:
            L = len(p)
            s, probes = backoff_model(tokens_abi.backoff_cap(L, backoff[1]),
                                      lambda k: np.subtract(*tokens_abi.range_definition(t, lst, p[L - k:])[::-1]), backoff[0])
        ctx = p[len(p) - s:] if s else []
        lo, hi, ae, listing = tokens_abi.next_tokens_definition(t, lst, ctx)
        cnt = hi - lo - ae
        searched = 0
        if cnt:
            run = [t[lst[i] + s] for i in range(lo + ae, hi)]
            got, slots = tokens_abi.stream_route_model(run, end)
            assert got == listing and slots == cnt
            got, searched = tokens_abi.search_route_model(run, end)
            assert got == listing
        rows.append((s, lo, hi, ae, [v for v, _ in listing], [c for _, c in listing], cnt, searched, probes))
    return rows


class TokenModel:
    """the token text (the shape of tests/test_tokens.py's Model, sized so that the whole expected listing stays below about
    16 M entries), its reference array, ten kinds of context and the lap batch over them"""

    def __init__(self, oracle, W):
        planted = np.empty(1200, dtype=np.uint16)
        planted[0::2] = HOT
        planted[1::2] = 1000 + np.arange(600)
        body = corpus.token_corpus(5000, 400, 9)
        edge = np.array([0xFFFF, 0xFFFF, 0, 0, 0xFFFF, 5, 0, 0xFFFF, 0], dtype=np.uint16)
        self.tok = tok = tokens_abi.as_tokens(np.concatenate((body[:2500], planted, edge, body[2500:], np.full(RUN_LEN, TOK_RUN))))
        tok.setflags(write=False)
        self.t = t = [int(x) for x in tok]
        self.n = n = len(t)
        self.arr = tokens_abi.reference_suffix_array(tok, oracle)
        self.arr.setflags(write=False)
        self.lst = lst = self.arr.tolist()

        def stripped(p):
            lo, hi, ae, _ = tokens_abi.next_tokens_definition(t, lst, p)
            return hi - lo - ae

        by_count = np.argsort(-np.bincount(body, minlength=65536), kind="stable")[:40]
        streamed = [[int(v)] for v in by_count if 256 < stripped([int(v)]) <= sa.NGRAM_STREAM_CAP_DEFAULT]
        short = [p for p in (t[100:102], t[1500:1501], t[4500:4503], t[200:230]) if 1 <= stripped(p) <= 64]
        assert len(streamed) >= 2 and len(short) >= 3
        image = tokens_abi.be_image(tok)
        odd = [[(int(image[a + 2 * i]) << 8) | int(image[a + 2 * i + 1]) for i in range(k)] for a, k in ((1, 1), (101, 2), (5001, 3), (8001, 2))]
        self.pools = [
            [[]],                                                     # the empty context
            streamed[:3],                                             # streamed, more than 256 slots
            short,                                                    # 1 to 64 slots
            [[50000, short[0][-1]], [HOT, 999], [7, 50001, short[1][-1]]],    # absent (a back-off ends in a short range, not in the empty context)
            [t, t[1:], t[3:]],                                        # the whole text
            [[TOK_RUN] * (RUN_LEN - 1), [TOK_RUN] * (RUN_LEN - 10), [TOK_RUN] * (RUN_LEN - 64)],      # ends the text and occurs elsewhere
            [[HOT]],                                                  # 600 continuations
            [[TOK_RUN], [TOK_RUN] * 2, [TOK_RUN] * 65, [TOK_RUN] * 300],      # inside the run
            [[0], [0xFFFF], [0xFFFF, 0xFFFF], [0, 0], [0, 0xFFFF]],   # tokens 0x0000 and 0xFFFF
            odd,                                                      # read from the byte image at odd offsets
        ]
        self.batch = Batch(W, [[np.array(p, dtype=np.uint16) for p in pool] for pool in self.pools], np.uint16)
        self.distinct = [p for pool in self.pools for p in pool]
        self._expected = {}
        rows = token_rows(t, lst, self.distinct, None)
        first = np.concatenate(([0], np.cumsum([len(p) for p in self.pools])))
        kinds = [rows[first[k]:first[k + 1]] for k in range(len(self.pools))]
        eff = sa.NGRAM_STREAM_CAP_DEFAULT
        assert kinds[0][0][1:4] == (0, n + 1, 1) and kinds[0][0][6] > eff and 256 < len(kinds[0][0][4]) <= 1500
        assert all(r[1] == r[2] for r in kinds[3]) and all(r[2] - r[1] == 1 and r[3] == 1 for r in kinds[4])
        assert all(r[3] == 1 and r[6] >= 1 and len(r[4]) == 1 for r in kinds[5])
        assert len(kinds[6][0][4]) == 600 and kinds[6][0][6] == 600
        assert all(r[6] > 256 and len(r[4]) == 1 for r in kinds[7]) and all(r[2] > r[1] for r in kinds[8])
        assert sum(r[1] == r[2] for r in kinds[9]) >= 2                # the image holds them, no token position does
        for p in odd:
            assert tokens_abi.be_image(tokens_abi.as_tokens(p)).tobytes() in image.tobytes()

    def expected(self, backoff):
        if backoff not in self._expected:
            self._expected[backoff] = Expected(self.batch, token_rows(self.t, self.lst, self.distinct, backoff), np.uint16)
            assert self._expected[backoff].total < 20 << 20
        return self._expected[backoff]


@pytest.fixture(scope="module")
def token_model(oracle):
    m = TokenModel(oracle, ngram_waves(cu_count()))
    built = sa.TokenIndex(m.tok)
    m.build_times = {k: sa.last_tok_stats()[k] for k in ("image_ms", "build_ms", "compact_ms")}
    given = sa.TokenIndex(m.tok, m.arr)
    m.indexes = (("built", TokIndex(built)), ("given", TokIndex(given)))
    try:
        yield m
    finally:
        built.close()
        given.close()


def test_token_search_over_three_laps(token_model):
    b, exp = token_model.batch, token_model.expected(None)
    for name, index in token_model.indexes:
        has = np.full(b.count + 2 * PAD, 0xA5, dtype=np.uint8)
        lo, hi = np.full(b.count + 2 * PAD, 0xA5A5A5A5, dtype=np.uint32), np.full(b.count + 2 * PAD, 0xA5A5A5A5, dtype=np.uint32)
        assert sa.lib().sa_amd_tok_index_search(index.ix._h, b.data.ctypes.data, b.off.ctypes.data, b.count, has[PAD:].ctypes.data,
                                                lo[PAD:].ctypes.data, hi[PAD:].ctypes.data) == 0
        for a in (has, lo, hi):
            raw = a.view(np.uint8)
            assert np.all(raw[:PAD * a.itemsize] == 0xA5) and np.all(raw[(PAD + b.count) * a.itemsize:] == 0xA5), name
        assert np.array_equal(lo[PAD:PAD + b.count], exp.lo) and np.array_equal(hi[PAD:PAD + b.count], exp.hi), name
        assert np.array_equal(has[PAD:PAD + b.count], (exp.hi > exp.lo).astype(np.uint8)), name


@pytest.mark.parametrize("cap", CAPS)
def test_next_tokens_over_three_laps(token_model, cap):
    exp = token_model.expected(None)
    for name, index in token_model.indexes:
        st = check_call(index, token_model.batch, exp, cap, None, (name, cap))
        assert st["compared_tokens"] == -1
        assert {k: st[k] for k in token_model.build_times} == token_model.build_times and st["build_ms"] > 0      # the build's times stay


@pytest.mark.parametrize("cap", CAPS)
def test_token_infgram_over_three_laps(token_model, cap):
    for backoff in BACKOFF:
        exp = token_model.expected(backoff)
        for name, index in token_model.indexes:
            st = check_call(index, token_model.batch, exp, cap, backoff, (name, cap, backoff))
            assert st["compared_tokens"] >= 0
            assert {k: st[k] for k in token_model.build_times} == token_model.build_times


@pytest.mark.parametrize("backoff", [None, (1, 0)], ids=["next_tokens", "infgram"])
def test_token_listing_cut_inside_a_query_of_the_second_lap(token_model, backoff):
    exp = token_model.expected(backoff)
    for name, index in token_model.indexes:
        check_capacity_cut(index, token_model.batch, exp, backoff, (name, backoff))


# ---------------------------------------------------------------- 3. byte against token, still one core ----


@pytest.mark.parametrize("cap", CAPS)
def test_the_two_instantiations_lap_alike(byte_model, cap):
    """the byte text and the token text holding the same values: equal ranges, listings and shared counters for the byte lap
    batch -- both sides against the byte definitions, their counters against each other"""
    b = byte_model.batch
    tb = Batch(b.W, [[_u8(p).astype(np.uint16) for p in pool] for pool in byte_model.pools], np.uint16)
    assert np.array_equal(tb.ids, b.ids) and np.array_equal(tb.off, b.off) and np.array_equal(tb.data, b.data)
    plain = byte_model.indexes[0][1]                                   # (no bucket table, no LCP table: the plain route on both sides)
    tok_ix = sa.TokenIndex(byte_model.t.astype(np.uint16))
    try:
        for backoff in (None, (2, 0)):
            exp = byte_model.expected(backoff)
            st_b = check_call(plain, b, exp, cap, backoff, ("bytes", cap, backoff))
            st_t = check_call(TokIndex(tok_ix), tb, exp, cap, backoff, ("tokens", cap, backoff))
            for k in SHARED_STATS:
                assert st_b[k] == st_t[k], (cap, backoff, k, st_b[k], st_t[k])
            assert st_b["compared_bytes"] == st_t["compared_tokens"], (cap, backoff)
    finally:
        tok_ix.close()


# ---------------------------------------------------------------- 4. documents ----

class DocsModel:
    """20 000 bytes of English in 300 documents, and a batch over a pool of four kinds of pattern -- no unit, one unit, tens of
    units, hundreds of units of DOC_CHUNK_MIN slots -- sized so that the units take more than three laps of the unit kernels,
    the patterns' scan has more than three tiles and the listing more than two laps of k_doc_tf"""

    def __init__(self, oracle, cu):
        self.t, self.tb = english(20000, 5)
        self.n = n = self.t.size
        self.arr = arr = oracle.sais(self.t)
        self.off = off = random_table(n, 300, 10)
        tb, chunk = self.tb, sa.DOC_CHUNK_MIN
        self.waves = docs_waves(cu)

        def occurrences(p):
            lo, hi = docs_abi.range_definition(tb, arr, p)
            return hi - lo

        rare = [p for p in (tb[1000:1006], tb[7000:7005], tb[15000:15008]) if 1 <= occurrences(p) <= chunk]
        self.pools = [[b"\x01\x02nope", b"zq\x00"], rare, [b"e"], [b""]]
        assert len(rare) >= 2
        self.distinct = [p for pool in self.pools for p in pool]
        occ, df, lists = docs_abi.answers_definition(tb, off, arr, self.distinct)
        self.tf = doc_tf_abi.answers_definition(tb, off, arr, self.distinct)
        for (o, ls, _), o2, l2 in zip(self.tf, occ, lists):
            assert o == o2 and np.array_equal(ls, l2)
        units = np.array([docs_abi.units_definition([o], chunk) for o in occ], dtype=np.int64)
        sizes = np.array([len(p) for p in self.pools])
        first = np.concatenate(([0], np.cumsum(sizes)))
        assert np.all(units[first[0]:first[1]] == 0) and np.all(units[first[1]:first[2]] == 1)
        assert 10 <= units[first[2]] < 100 <= units[first[3]]
        group_units = int(units[first[:-1]].sum())                     # per four patterns: 0 + 1 + tens + hundreds
        group_entries = int(min(df[first[1]:first[2]])) + int(df[first[2]]) + int(df[first[3]])
        m = 1 + max(-(-(3 * self.waves + 37) // group_units), -(-(3 * DOC_SCAN_TILE + 1) // 4), -(-(2 * doc_tf_lanes(cu) + 1) // group_entries))
        q = np.arange(4 * m, dtype=np.int64)
        self.kind = q % 4
        self.ids = first[self.kind] + (q // 4) % sizes[self.kind]
        self.count = int(q.size)
        self.pats = [self.distinct[i] for i in self.ids.tolist()]
        self.occ, self.df, self.units = occ[self.ids], df[self.ids], units[self.ids]
        self.loff, self.docs = gather(*pool_of(lists, np.int64), self.ids)
        _, self.tfs = gather(*pool_of([a[2] for a in self.tf], np.int64), self.ids)
        top = [doc_tf_abi.topk_definition(a[1], a[2], 5) for a in self.tf]
        self.toff, self.top_docs = gather(*pool_of([d for d, _ in top], np.int64), self.ids)
        _, self.top_tf = gather(*pool_of([f for _, f in top], np.int64), self.ids)
        # the flagged slots of every distinct pattern, relative to its range: where the listing's entries come from
        self.flagged = []
        for p in self.distinct:
            lo, hi = docs_abi.range_definition(tb, arr, p)
            d = docs_abi.doc_of_definition(off, n, np.asarray(arr[lo:hi], dtype=np.int64))
            seen = np.flatnonzero(d != docs_abi.NONE)
            _, firsts = np.unique(d[seen], return_index=True)
            self.flagged.append(np.sort(seen[firsts]))
        # the sizes this model is for
        assert int(self.units.sum()) >= 3 * self.waves + 37
        assert self.count + 1 > 3 * DOC_SCAN_TILE and int(self.units.sum()) + 1 > 3 * DOC_SCAN_TILE
        assert int(self.loff[-1]) > 2 * doc_tf_lanes(cu)


@pytest.fixture(scope="module")
def docs_model(oracle):
    m = DocsModel(oracle, cu_count())
    ix = sa.DeviceIndex(m.t, m.arr)
    ix.set_documents(m.off)
    ix.enable_doc_freq()
    m.ix = ix
    try:
        yield m
    finally:
        ix.close()


@contextlib.contextmanager
def smallest_chunk():
    """units of DOC_CHUNK_MIN slots for the calling thread, the previous value restored behind the block"""
    prev = sa.docs_set_chunk(sa.DOC_CHUNK_MIN)
    try:
        yield
    finally:
        sa.docs_set_chunk(prev)


def test_doc_search_and_doc_list_over_three_laps_of_units(docs_model):
    m = docs_model
    assert docs_abi.units_definition(m.occ, sa.DOC_CHUNK_MIN) == int(m.units.sum()) >= 3 * m.waves + 37      # before the call
    with smallest_chunk():
        occ, df = m.ix.doc_search(m.pats)
        st = sa.last_docs_stats()
        total, loff, docs = raw_list(m.ix, m.pats, int(m.loff[-1]) + 5)
        st2 = sa.last_docs_stats()
    assert np.array_equal(occ, m.occ) and np.array_equal(df, m.df)
    want = {"patterns": m.count, "occ_sum": int(m.occ.sum()), "units": int(m.units.sum()), "df_sum": int(m.df.sum()),
            "slots_scanned": int(m.occ.sum()), "chunk": sa.DOC_CHUNK_MIN, "readbacks": 1, "listed": 0}
    assert st == want, (st, want)
    assert total == m.loff[-1] and np.array_equal(loff, m.loff)
    bad = np.flatnonzero(docs != m.docs)
    assert bad.size == 0, (int(bad.size), (np.searchsorted(m.loff, bad[:4], "right") - 1).tolist())
    want.update(slots_scanned=2 * int(m.occ.sum()), listed=1)
    assert st2 == want, (st2, want)


def test_doc_listing_cut_inside_a_unit_of_the_second_lap(docs_model):
    m = docs_model
    chunk = sa.DOC_CHUNK_MIN
    uoff = np.concatenate(([0], np.cumsum(m.units)))
    # a pattern of hundreds of units whose first unit a wave reaches on its second lap, and a unit of it with two entries or more
    cand = np.flatnonzero((m.kind == 3) & (uoff[:-1] >= m.waves) & (uoff[:-1] + 4 < 2 * m.waves))
    assert cand.size
    q = int(cand[cand.size // 2])
    fl = m.flagged[int(m.ids[q])]
    per_unit = np.bincount(fl // chunk, minlength=int(m.units[q]))
    k = int(np.flatnonzero(per_unit[:4] >= 2)[-1])
    u = int(uoff[q]) + k
    assert m.waves <= u < 2 * m.waves
    capacity = int(m.loff[q] + per_unit[:k].sum() + per_unit[k] // 2)
    assert m.loff[q] < capacity < m.loff[q + 1]
    with smallest_chunk():
        total, loff, docs = raw_list(m.ix, m.pats, capacity)          # (raw_list: nothing before, nothing past what fits)
        st = sa.last_docs_stats()
    assert total == m.loff[-1] and np.array_equal(loff, m.loff) and docs.size == capacity
    assert np.array_equal(docs, m.docs[:capacity])
    assert st["df_sum"] == total and st["units"] == int(m.units.sum()) and st["occ_sum"] == int(m.occ.sum())


def test_doc_tf_and_doc_topk_over_two_laps_of_entries(docs_model):
    m = docs_model
    with smallest_chunk():
        total, loff, docs, tf = raw_tf(m.ix, m.pats, int(m.loff[-1]) + 5)
        st = sa.last_doc_tf_stats()
        toff, top_docs, top_tf = raw_topk(m.ix, m.pats, 5)
        st2 = sa.last_doc_tf_stats()
    assert total == m.loff[-1] > 2 * doc_tf_lanes(cu_count()) and np.array_equal(loff, m.loff)
    assert np.array_equal(docs, m.docs)
    bad = np.flatnonzero(tf != m.tfs)
    assert bad.size == 0, (int(bad.size), bad[:4].tolist(), (np.searchsorted(m.loff, bad[:4], "right") - 1).tolist())
    want = {"patterns": m.count, "occ_sum": int(m.occ.sum()), "df_sum": total, "tf_sum": int(m.tfs.sum()), "topk_entries": 0, "pieces": 0,
            "rounds": 0, "k": 0, "piece": 0, "chunk": sa.DOC_CHUNK_MIN}
    assert {f: st[f] for f in want} == want, (st, want)
    assert np.array_equal(toff, m.toff) and np.array_equal(top_docs, m.top_docs) and np.array_equal(top_tf, m.top_tf)
    P = doc_tf_abi.effective_piece(sa.DOC_TOPK_PIECE_DEFAULT, 5)
    rounds, pieces, final = doc_tf_abi.plan_definition(np.diff(m.loff), P, 5)
    want.update(topk_entries=int(m.toff[-1]), pieces=pieces, rounds=rounds, k=5, piece=P)
    assert {f: st2[f] for f in want} == want, (st2, want)
    assert final == np.diff(m.toff).tolist()


# ---------------------------------------------------------------- 5. the token build past its laps ----

@functools.lru_cache(maxsize=None)
def big_tokens(family):
    """-> (the text of tok_build_size tokens, its reference array, the entries the compaction keeps on its second lap):
    computed once, shared, never changed.  The reference is reference_suffix_array's route above BRUTE_MAX tokens."""
    from conftest import Oracle
    cu = cu_count()
    t = tokens_abi.families(tok_build_size(cu))[family]
    t.setflags(write=False)
    assert t.size > tokens_abi.BRUTE_MAX
    byte_sa = Oracle().sais(tokens_abi.be_image(t))
    ref = tokens_abi.even_entries_halved(byte_sa)
    ref.setflags(write=False)
    return t, ref, int(np.count_nonzero((byte_sa[tok_compact_lap(cu):] & 1) == 0))


@pytest.mark.parametrize("family", ["zipf_50000", "below_256", "fibonacci", "multiples_of_256"])
def test_token_build_past_one_compaction_lap(family):
    """2 n + 1 is just past one lap of the compaction kernels with a partial last span, the image pass is in its third lap, the
    count scan has five tiles and the byte builder is past gram_min_n (tests/test_grid_laps_abi.py pins all four).  The end of
    the byte-level array holds the suffixes with the largest first byte: under zipf_50000 (no high byte 0xFF), below_256 (every
    high byte zero) and fibonacci (the largest suffixes start inside a token) all of these start at odd offsets, so the second
    lap of the compaction counts zeros and scatters nothing.  Under multiples_of_256 (every low byte zero) all of them start at
    even offsets: the second lap's counts, their place in the scan and its scatter carry the end of the token array."""
    t, ref, kept_on_second_lap = big_tokens(family)
    assert t.size == tok_build_size(cu_count()) and ref.size == t.size + 1
    if family == "multiples_of_256":
        assert kept_on_second_lap == 2 * t.size + 1 - tok_compact_lap(cu_count()) > 3 * TK_TILE
    for how, got in (("saca_u16", _saca_u16_canaried(t)), ("index", None)):
        if got is None:
            ix = sa.TokenIndex(t)
            got = ix.sa()
            ix.close()
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (family, how, int(bad.size), bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())
    st = sa.last_tok_stats()
    assert st["image_ms"] >= 0 and st["build_ms"] > 0 and st["compact_ms"] > 0


@pytest.mark.parametrize("where", ["correct", "slot_7", "second_lap", "last_slot", "swapped"])
def test_range_check_of_a_supplied_array_past_its_first_lap(where):
    """k_tok_sa_range is the only guard between a caller's array and every later read through it: one bad entry (n + 1) in its
    first lap, one in its second and one in the last slot are each refused with -6; entries 0 and 1 swapped (in range, but
    SA[0] != n) with -1; the reference array is taken.  No query is run on any of these."""
    t, ref, _ = big_tokens("fibonacci")
    n = t.size
    lap = tok_range_lap(cu_count())
    assert 7 < lap and lap + 5 < n
    if where == "correct":
        sa.TokenIndex(t, ref).close()
        return
    bad = ref.copy()
    if where == "swapped":
        bad[0], bad[1] = bad[1], bad[0]
    else:
        bad[{"slot_7": 7, "second_lap": lap + 5, "last_slot": n}[where]] = n + 1
    with pytest.raises(sa.SuffixArrayError) as e:
        sa.TokenIndex(t, bad)
    assert e.value.code == (-1 if where == "swapped" else -6)
