"""CPU suite for the 16-bit token texts (kernels/tokens.hpp, host/tokens.hpp): the definitions restated in
numpy over a brute-force token suffix array, the argument for the construction route (the suffix array of the BIG-endian byte
image, its even entries halved -- and not the little-endian image), a model of the compaction (tile counts, scan, scatter), models
of the two continuation routes with their probe bound at listings below, at and above 256 entries, the header's example, the
exports and the Python surface, and the argument checks that answer without a device.  tests/test_tokens.py imports the
definitions and the text families from here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT

EXPORTS = ("sa_amd_max_tokens_u16", "sa_amd_saca_u16", "sa_amd_tok_index_create", "sa_amd_tok_index_destroy", "sa_amd_tok_index_sa",
           "sa_amd_tok_index_search", "sa_amd_tok_index_next_tokens", "sa_amd_tok_index_infgram", "sa_amd_last_tok_stats")
STATS_FIELDS = ("patterns", "range_searches", "compared_tokens", "stream_slots", "search_slots", "stream_queries", "search_queries",
                "empty_queries", "entries", "stream_cap", "readbacks", "backoff", "passes", "image_ms", "build_ms", "compact_ms")
EXAMPLE_TEXT = [256, 1, 256, 1, 2]
EXAMPLE_SA = [5, 3, 1, 4, 2, 0]
WAVE = 64
LOADS = 4                     # NG_LOADS: loads a lane of the streaming route has in flight
END = 65536                   # TK_END
BRUTE_MAX = 2000


def kernel_constant(name):
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "tokens.hpp")) as f:
        m = re.search(r"constexpr int " + name + r" = (\d+);", f.read())
    assert m, name
    return int(m.group(1))


TILE = 2048                   # TK_TILE: entries of the byte-level array per count (test_compaction_constants pins both)
SPAN = 4                      # TK_SPAN: tiles a workgroup takes in one trip


def ceil_log2(x):
    return 0 if x <= 1 else (x - 1).bit_length()


# ---------------------------------------------------------------- the definitions ----

def as_tokens(t):
    return np.ascontiguousarray(t, dtype=np.uint16)


def brute_suffix_array(tokens):
    """the definition: token suffixes in the order of Python's list comparison -- unsigned values, a proper prefix first"""
    t = [int(x) for x in tokens]
    assert len(t) <= BRUTE_MAX
    return np.array(sorted(range(len(t) + 1), key=lambda i: t[i:]), dtype=np.uint32)


def be_image(tokens):
    return as_tokens(tokens).astype(">u2").view(np.uint8).copy()


def le_image(tokens):
    return as_tokens(tokens).astype("<u2").view(np.uint8).copy()


def even_entries_halved(byte_sa):
    a = np.asarray(byte_sa, dtype=np.uint32)
    return (a[(a & 1) == 0] >> 1).astype(np.uint32)


def reference_suffix_array(tokens, oracle):
    """brute force where it is affordable, else the route the CPU suite pins: the oracle on the big-endian image"""
    if len(tokens) <= BRUTE_MAX:
        return brute_suffix_array(tokens)
    return even_entries_halved(oracle.sais(be_image(tokens)))


def range_definition(t, arr, pat):
    """[lo, hi): the slots whose suffix starts with pat; lo == hi == the number of smaller suffixes where there is none.
    t: list of ints, arr: the token suffix array.  Two binary searches on the first len(pat) tokens of the suffixes."""
    p, N1 = len(pat), len(arr)
    lo, hi = 0, N1
    while lo < hi:
        m = (lo + hi) // 2
        if t[arr[m]:arr[m] + p] < pat:
            lo = m + 1
        else:
            hi = m
    lo2, hi2 = lo, N1
    while lo2 < hi2:
        m = (lo2 + hi2) // 2
        if t[arr[m]:arr[m] + p] == pat:
            lo2 = m + 1
        else:
            hi2 = m
    return lo, lo2


def brute_range(t, arr, pat):
    """the same by looking at every slot"""
    p = len(pat)
    hits = [i for i in range(len(arr)) if t[arr[i]:arr[i] + p] == pat]
    if hits:
        assert hits == list(range(hits[0], hits[-1] + 1))
        return hits[0], hits[-1] + 1
    below = sum(1 for i in range(len(arr)) if t[arr[i]:] < pat)
    return below, below


def next_tokens_definition(t, arr, pat):
    """-> (lo, hi, at_end, listing): the header's definition; listing = [(token, count)] ascending"""
    n, p = len(t), len(pat)
    lo, hi = range_definition(t, arr, pat)
    ends = [i for i in range(lo, hi) if arr[i] + p == n]
    assert ends in ([], [lo])                                         # at_end can only be slot lo
    conts = [t[arr[i] + p] for i in range(lo + len(ends), hi)]
    assert conts == sorted(conts)                                     # the sub-range identity's ground
    vals, counts = np.unique(np.array(conts, dtype=np.int64), return_counts=True)
    listing = [(int(v), int(c)) for v, c in zip(vals, counts)]
    assert sum(c for _, c in listing) + len(ends) == hi - lo
    return lo, hi, len(ends), listing


def backoff_cap(L, max_len):
    return L if max_len <= 0 else min(L, max_len)


def infgram_definition(t, arr, prompt, min_count, max_len):
    """-> (s, lo, hi, at_end, listing): the largest s in 0 .. cap whose suffix of the prompt has at least min_count occurrences"""
    L = len(prompt)
    for s in range(backoff_cap(L, max_len), -1, -1):
        ctx = prompt[L - s:]
        lo, hi = range_definition(t, arr, ctx)
        if s == 0 or hi - lo >= min_count:
            return (s,) + next_tokens_definition(t, arr, ctx)
    raise AssertionError


# ---------------------------------------------------------------- the text families ----

def fibonacci_tokens(n, a=1, b=256):
    x, y = [a], [a, b]
    while len(y) < n:
        x, y = y, y + x
    return y[:n]


def families(n, seed=0):
    """name -> n tokens; every family the construction is tested on"""
    rng = np.random.default_rng(seed + 7 * n)
    out = {
        "one_token": np.full(n, 0x0100),
        "period_2": np.resize(np.array([0x0100, 0x0001]), n),
        "below_256": rng.integers(0, 256, n),
        "multiples_of_256": rng.integers(0, 256, n) * 256,
        "zeros_and_ffff": np.where(rng.random(n) < 0.5, 0x0000, 0xFFFF),
        "fibonacci": np.array(fibonacci_tokens(n), dtype=np.int64) if n else np.zeros(0, dtype=np.int64),
        "zipf_50000": corpus.token_corpus(n, 50000, seed + 1),
    }
    return {k: as_tokens(v) for k, v in out.items()}


SMALL_SIZES = (0, 1, 2, 3, 5, 64, 65, 257, 700)


def small_cases():
    yield "header", as_tokens(EXAMPLE_TEXT)
    for n in SMALL_SIZES:
        for name, t in families(n).items():
            yield f"{name}_{n}", t


# ---------------------------------------------------------------- the route ----

def test_header_example_is_the_brute_force_array():
    assert brute_suffix_array(EXAMPLE_TEXT).tolist() == EXAMPLE_SA


def test_big_endian_image_route_gives_the_token_order(oracle):
    """oracle.sais of the big-endian image, filtered to even entries and halved, is the brute-force array on every case"""
    seen = 0
    for name, t in small_cases():
        byte_sa = oracle.sais(be_image(t))
        assert byte_sa.size == 2 * t.size + 1
        got = even_entries_halved(byte_sa)
        assert got.size == t.size + 1 and got[0] == t.size, name
        assert np.array_equal(got, brute_suffix_array(t)), name
        seen += 1
    assert seen == 1 + len(SMALL_SIZES) * 7


def test_little_endian_image_does_not(oracle):
    """the negative check: on the header example the little-endian image gives ANOTHER order (0x0100 before 0x0001), so a test
    that passes with either endianness shows nothing -- this text tells them apart"""
    t = as_tokens(EXAMPLE_TEXT)
    got = even_entries_halved(oracle.sais(le_image(t)))
    assert got.size == t.size + 1
    assert got.tolist() != EXAMPLE_SA
    assert even_entries_halved(oracle.sais(be_image(t))).tolist() == EXAMPLE_SA


def test_token_corpus_is_seeded_and_zipf():
    a, b = corpus.token_corpus(5000, 50000, 3), corpus.token_corpus(5000, 50000, 3)
    assert a.dtype == np.uint16 and a.shape == (5000,) and np.array_equal(a, b)
    assert not np.array_equal(a, corpus.token_corpus(5000, 50000, 4))
    assert np.unique(a).size > 256                                    # more than 256 distinct continuations of the empty context
    assert int(np.max(a >> 8)) > 0 and corpus.token_corpus(0, 10, 1).size == 0
    assert int(corpus.token_corpus(4000, 100, 1).max()) < 100
    with pytest.raises(ValueError):
        corpus.token_corpus(10, 70000, 1)


# ---------------------------------------------------------------- the compaction ----

def compaction_model(byte_sa, tile=TILE, span=SPAN):
    """k_tok_compact_count, the scan, k_tok_compact_scatter: per tile the number of even entries, an exclusive scan over
    tiles + 1 words, then per tile the kept entries, halved, at the tile's offset plus their rank inside the tile.  A workgroup
    takes `span` tiles a trip, which must not show."""
    a = np.asarray(byte_sa, dtype=np.uint32)
    tiles = -(-a.size // tile)
    cnt = np.zeros(tiles + 1, dtype=np.int64)
    for sp in range(-(-tiles // span)):
        for k in range(span):
            tl = sp * span + k
            if tl < tiles:
                cnt[tl] = int(np.count_nonzero((a[tl * tile:(tl + 1) * tile] & 1) == 0))
    off = np.concatenate(([0], np.cumsum(cnt)[:-1]))
    out = np.full(int(off[tiles]), 0xFFFFFFFF, dtype=np.uint32)
    for tl in range(tiles):
        part = a[tl * tile:(tl + 1) * tile]
        keep = (part & 1) == 0
        rank = np.cumsum(keep) - keep                                 # (what the ballots and popcounts compute, wave by wave)
        out[off[tl] + rank[keep]] = part[keep] >> 1
    return out


def test_compaction_constants():
    assert (kernel_constant("TK_THREADS"), kernel_constant("TK_LOADS"), kernel_constant("TK_SPAN")) == (256, 2, SPAN)
    assert 256 // WAVE * kernel_constant("TK_LOADS") * WAVE * 4 == TILE      # waves x loads x one 16-byte load of a wave
    assert kernel_constant("TK_END") == END


@pytest.mark.parametrize("n1", [1, 2, TILE // 2, TILE // 2 + 1, TILE - 1, TILE, TILE + 1, SPAN * TILE - 1, SPAN * TILE, SPAN * TILE + 1, 3 * SPAN * TILE + 77])
def test_compaction_model_is_the_filter(n1):
    """n + 1 around one tile and one span of tiles (in entries of the byte-level array and in kept entries)"""
    n = n1 - 1
    rng = np.random.default_rng(n1)
    byte_sa = rng.permutation(2 * n + 1).astype(np.uint32)            # any arrangement of 0 .. 2 n: n + 1 even entries
    got = compaction_model(byte_sa)
    assert got.size == n + 1 and np.array_equal(got, even_entries_halved(byte_sa))
    assert np.array_equal(compaction_model(byte_sa, 64, 3), got)


# ---------------------------------------------------------------- the continuation routes ----

def stream_route_model(run, end=END):
    """the streaming route of k_tok_next: the range is read once, LOADS * 64 slots a trip; a lane compares its token with its
    left neighbour's; ranks from the ballot of the listed starts, counts from the next set bit of the ballot of all starts, the
    last start of a ballot waits for the first start of a later one.  end: the sentinel sym_end<Sym>(), 65 536 at 16 bits and
    2^24 at 32.  -> (listing, slots probed)"""
    cnt = len(run)
    toks, counts = {}, {}
    listed, carry, pend = 0, -1, None
    for r in range(0, cnt, LOADS * WAVE):
        for k in range(LOADS):
            first = r + k * WAVE
            b = [run[first + l] if first + l < cnt else end for l in range(WAVE)]
            left = [carry] + b[:-1]
            carry = b[-1]
            start = [first + l < cnt and b[l] != left[l] for l in range(WAVE)]
            lst = [start[l] and b[l] < end for l in range(WAVE)]
            if not any(start):
                continue
            starts = [l for l in range(WAVE) if start[l]]
            if pend is not None:
                counts[pend[0]] = first + starts[0] - pend[1]
            for l in starts:
                if lst[l]:
                    rank = listed + sum(lst[:l])
                    toks[rank] = b[l]
                    above = [x for x in starts if x > l]
                    if above:
                        counts[rank] = above[0] - l
            last = starts[-1]
            pend = (listed + sum(lst[:last]), first + last) if lst[last] else None
            listed += sum(lst)
    if pend is not None:
        counts[pend[0]] = cnt - pend[1]
    assert sorted(toks) == sorted(counts) == list(range(listed))
    return [(toks[i], counts[i]) for i in range(listed)], cnt


def search_route_model(run, end=END):
    """the boundary-search route: lane l probes the sample slot l (cnt - 1) / 63; between two samples with different tokens a
    lane finds every run start by one binary search for the first slot with a token above the last one found.  A lane's ranks
    start at the exclusive sum of the starts of the lanes before it; its last run ends at the first start of a later lane.
    end: as in stream_route_model.  -> (listing, slots probed)"""
    cnt = len(run)
    pos = [l * (cnt - 1) // (WAVE - 1) for l in range(WAVE)]
    probes = WAVE
    found = []                                                        # per lane: [(place, token)]
    for l in range(WAVE):
        mine = [(0, run[0])] if l == 0 else []
        if l < WAVE - 1:
            x, a, bn, posn = run[pos[l]], pos[l], run[pos[l + 1]], pos[l + 1]
            while x < bn:
                u, v, bv = a + 1, posn, bn
                while u < v:
                    m = u + (v - u) // 2
                    probes += 1
                    if run[m] > x:
                        v, bv = m, run[m]
                    else:
                        u = m + 1
                mine.append((u, bv))
                x, a = bv, u
        found.append(mine)
    listing = []
    for l in range(WAVE):
        later = [f[0][0] for f in found[l + 1:] if f]
        for j, (at, tok) in enumerate(found[l]):
            nxt = found[l][j + 1][0] if j + 1 < len(found[l]) else (later[0] if later else cnt)
            if tok < end:
                listing.append((tok, nxt - at))
    return listing, probes


def search_route_bound(cnt, distinct):
    return WAVE + distinct * (ceil_log2(cnt + 1) + 1)


def listing_of_run(run):
    vals, counts = np.unique(np.array([x for x in run if x < END], dtype=np.int64), return_counts=True)
    return [(int(v), int(c)) for v, c in zip(vals, counts)]


def sorted_run(rng, distinct, cnt, vocab=65536):
    """cnt >= distinct continuation tokens in ascending order with exactly `distinct` values"""
    vals = np.sort(rng.choice(vocab, distinct, replace=False))
    extra = np.sort(rng.integers(0, distinct, cnt - distinct))
    return [int(x) for x in np.sort(np.concatenate((vals, vals[extra])))]


@pytest.mark.parametrize("distinct", [1, 2, 255, 256, 257, 1000])
def test_route_models_and_their_bound(distinct):
    """both routes give the definition's listing, the streaming route probes cnt slots and the boundary search at most
    64 + D (ceil(log2(cnt + 1)) + 1) -- for listings below, at and above the 256 entries a byte listing ends at"""
    rng = np.random.default_rng(distinct)
    for cnt in sorted({distinct, distinct + 1, 2 * distinct + 63, 64, 65, 4 * WAVE * LOADS + 1, 5000} | {max(distinct, 257)}):
        if cnt < distinct:
            continue
        for vocab in (65536, max(distinct, 300)):
            run = sorted_run(rng, distinct, cnt, vocab)
            want = listing_of_run(run)
            assert len(want) == distinct
            got, probed = stream_route_model(run)
            assert got == want and probed == cnt
            got, probed = search_route_model(run)
            assert got == want, (distinct, cnt)
            assert probed <= search_route_bound(cnt, distinct), (distinct, cnt, probed)
    # a run of END behind the tokens (only an array that is no suffix array has one): it ends the last run and is not listed
    run = sorted_run(rng, distinct, distinct + 70) + [END] * 5
    assert stream_route_model(run)[0] == listing_of_run(run) == search_route_model(run)[0]


# ---------------------------------------------------------------- the header's example and the definitions ----

def test_the_header_example():
    t, arr = EXAMPLE_TEXT, EXAMPLE_SA
    rows = {(256, 1): (4, 6, 0, [(2, 1), (256, 1)]), (1,): (1, 3, 0, [(2, 1), (256, 1)]), (2,): (3, 4, 1, []),
            (): (0, 6, 1, [(1, 2), (2, 1), (256, 2)])}
    for ctx, want in rows.items():
        assert next_tokens_definition(t, arr, list(ctx)) == want, ctx
    lo, hi, ae, listing = next_tokens_definition(t, arr, [9])
    assert lo == hi and ae == 0 and listing == []
    prompt = [7, 256, 1]
    assert infgram_definition(t, arr, prompt, 1, 0)[:3] == (2, 4, 6)
    assert infgram_definition(t, arr, prompt, 3, 0)[:3] == (0, 0, 6)
    assert infgram_definition(t, arr, prompt, 2, 1)[:3] == (1, 1, 3)
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for row in ("T = {256, 1, 256, 1, 2}, SA = {5, 3, 1, 4, 2, 0}", "{256, 1} [4, 6) 0 {2:1, 256:1}", "{1} [1, 3) 0 {2:1, 256:1}",
                "{2} [3, 4) 1 empty", "{} [0, 6) 1 {1:2, 2:1, 256:2}", "{9} empty 0 empty", "{7, 256, 1} 1 none 2 [4, 6)",
                "{7, 256, 1} 3 none 0 [0, 6)", "{7, 256, 1} 2 1 1 [1, 3)"):
        assert row in header.replace(" * ", " "), row


def contexts_of(t, rng):
    n = len(t)
    out = [[], [9], [65535], [0]]
    for _ in range(12):
        if n:
            a = int(rng.integers(0, n))
            k = int(rng.integers(1, 6))
            out.append(t[a:a + k])
            out.append(t[a:a + k] + [int(rng.integers(0, 65536))])
    out.append(t[max(n - 2, 0):])                                     # a suffix of the text: at_end
    out.append(list(t))                                               # the whole text
    out.append(list(t) + [1])                                         # longer than the text
    return out


def test_definitions_against_brute_force():
    rng = np.random.default_rng(5)
    for name, tok in small_cases():
        if tok.size > 300:
            continue
        t = [int(x) for x in tok]
        arr = brute_suffix_array(t).tolist()
        for ctx in contexts_of(t, rng):
            assert range_definition(t, arr, ctx) == brute_range(t, arr, ctx), (name, ctx[:8])
            lo, hi, ae, listing = next_tokens_definition(t, arr, ctx)
            at = lo + ae
            for v, c in listing:                                      # the sub-range identity: the range of ctx + [v]
                assert brute_range(t, arr, ctx + [v]) == (at, at + c), (name, ctx[:8], v)
                at += c
            assert at == hi
        for prompt in contexts_of(t, rng):
            for min_count, max_len in ((1, 0), (2, 0), (3, 2), (len(t) + 2, 0)):
                s, lo, hi, ae, listing = infgram_definition(t, arr, prompt, min_count, max_len)
                assert s <= backoff_cap(len(prompt), max_len) and (s == 0 or hi - lo >= min_count)
                if s < backoff_cap(len(prompt), max_len):
                    r = brute_range(t, arr, prompt[len(prompt) - s - 1:])
                    assert r[1] - r[0] < min_count


# ---------------------------------------------------------------- the surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    body = header[header.index("typedef struct sa_amd_tok_stats"):header.index("} sa_amd_tok_stats;")]
    declared = re.findall(r"^\s+(int64_t|int32_t|double)\s+(\w+);", body, re.M)
    assert [name for _, name in declared] == list(STATS_FIELDS) == [name for name, _ in sa.TokStats._fields_]
    size = {"int64_t": 8, "int32_t": 4, "double": 8}
    for (ctype_name, name), (_, ctype) in zip(declared, sa.TokStats._fields_):
        assert ctypes.sizeof(ctype) == size[ctype_name], name
    assert ctypes.sizeof(sa.TokStats) == 9 * 8 + 4 * 4 + 3 * 8
    # the token forms have no `void *stream` parameter: a device form comes with its stream test
    plain = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, params in re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", plain):
        if "tok" in name or name.endswith("_u16"):
            assert "stream" not in params, name
    assert L.sa_amd_max_tokens_u16() == sa.MAX_TOKENS_U16 == (2**31 - 1) // 2 == 1073741823


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for name in ("saca_u16", "MAX_TOKENS_U16", "TokenIndex", "TokStats", "last_tok_stats"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert params(sa.saca_u16) == ["tokens"] and params(sa.TokenIndex.__init__) == ["self", "tokens", "sa"]
    assert inspect.signature(sa.TokenIndex.__init__).parameters["sa"].default is None
    for op in ("sa", "search", "count", "contains", "next_tokens", "infgram"):
        assert callable(getattr(sa.TokenIndex, op)), op
    assert params(sa.TokenIndex.search) == params(sa.TokenIndex.next_tokens) == ["self", "patterns"]
    assert params(sa.TokenIndex.infgram) == ["self", "prompts", "min_count", "max_len"]
    assert [inspect.signature(sa.TokenIndex.infgram).parameters[k].default for k in ("min_count", "max_len")] == [1, 0]
    assert set(sa.last_tok_stats()) == set(STATS_FIELDS)
    assert params(corpus.token_corpus) == ["n", "vocab", "seed"]


def test_python_rejects_bad_tokens_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sa, "lib", no_library)
    for bad, err in (([1, 65536], ValueError), ([-1], ValueError), ([1.5], TypeError), (["a"], TypeError), (b"ab", TypeError),
                     (np.zeros(3, dtype=np.uint8), TypeError), (np.zeros(3, dtype=np.int32), TypeError),
                     (np.zeros((2, 2), dtype=np.uint16), TypeError), ([True], TypeError)):
        with pytest.raises(err):
            sa.saca_u16(bad)
        with pytest.raises(err):
            sa.TokenIndex(bad)
        with pytest.raises(err):
            sa._token_batch([[1, 2], bad])
    data, off, cnt = sa._token_batch([[1, 2], np.array([65535], dtype=np.uint16), []])
    assert data.dtype == np.uint16 and data.tolist() == [1, 2, 65535] and off.tolist() == [0, 2, 3, 3] and cnt == 3
    data, off, cnt = sa._token_batch([])
    assert data.size >= 1 and off.tolist() == [0] and cnt == 0


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    g = good.ctypes.data
    assert L.sa_amd_tok_index_search(None, p, g, 2, p, p, p) == -1                                    # NULL index
    assert L.sa_amd_tok_index_next_tokens(None, p, g, 2, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_tok_index_infgram(None, p, g, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_tok_index_sa(None, p) == -1 and L.sa_amd_tok_index_sa(fake, None) == -1
    assert L.sa_amd_tok_index_search(fake, p, g, -1, p, p, p) == -1                                   # negative count, capacity
    assert L.sa_amd_tok_index_next_tokens(fake, p, g, -1, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_tok_index_next_tokens(fake, p, g, 2, p, p, p, p, p, p, -1, c) == -1
    assert L.sa_amd_tok_index_infgram(fake, p, g, -1, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_tok_index_infgram(fake, p, g, 2, 1, 0, p, p, p, p, p, p, p, -1, c) == -1
    for min_count in (0, -1, -2**31):                                                                 # min_count < 1
        assert L.sa_amd_tok_index_infgram(fake, p, g, 2, min_count, 0, p, p, p, p, p, p, p, 4, c) == -1
    assert L.sa_amd_tok_index_next_tokens(fake, p, None, 2, p, p, p, p, p, p, 4, c) == -1             # pat_off as the search rejects it
    assert L.sa_amd_tok_index_next_tokens(fake, None, g, 2, p, p, p, p, p, p, 4, c) == -1
    for off in bad:
        assert L.sa_amd_tok_index_search(fake, p, off.ctypes.data, 2, p, p, p) == -1
        assert L.sa_amd_tok_index_next_tokens(fake, p, off.ctypes.data, 2, p, p, p, p, p, p, 4, c) == -1
        assert L.sa_amd_tok_index_infgram(fake, p, off.ctypes.data, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == -1
    h = ctypes.c_void_p(p)
    for n in (-1, sa.MAX_TOKENS_U16 + 1, 2**31 - 1):                                                  # n < 0, n above the maximum
        assert L.sa_amd_saca_u16(p, p, n) == -1
        assert L.sa_amd_tok_index_create(p, n, None, ctypes.byref(h)) == -1
    assert L.sa_amd_saca_u16(None, p, 3) == -1 and L.sa_amd_saca_u16(p, None, 3) == -1 and L.sa_amd_saca_u16(None, None, 0) == -1
    assert L.sa_amd_tok_index_create(None, 3, None, ctypes.byref(h)) == -1 and L.sa_amd_tok_index_create(p, 3, None, None) == -1
    assert tot.value == -5 and np.all(buf == 0x77777777)
    one = np.full(3, 0x55555555, dtype=np.uint32)
    assert L.sa_amd_saca_u16(None, one.ctypes.data, 0) == 0 and one.tolist() == [0, 0x55555555, 0x55555555]      # n == 0: SA = {0}
    L.sa_amd_last_tok_stats(None)
    L.sa_amd_tok_index_destroy(None)
    with pytest.raises(sa.SuffixArrayError):
        sa.TokenIndex.infgram(object.__new__(sa.TokenIndex), [[1]], min_count=0)
